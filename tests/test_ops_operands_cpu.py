"""The host-side operand checks of avdino.ops and the arguments its wrappers hand to the library
(no GPU: CPU tensors, ops.call / ops.stream replaced by a recorder).

Part one: the row-block checker at its edges.  Part two: every wrapper that takes a strided
block of rows or a flat buffer is called once with non-zero offsets and ld > cols, and the whole
recorded argument tuple is compared with one written out here from the parameter lists of
include/avdino.h: pointers are base.data_ptr() + element_size * offset, scalars are as passed."""
import pytest
import torch

STREAM = 0x5EED


# ------------------------------------------------------------------ part one: the row-block checker
ROWS, COLS, LD, OFF = 3, 8, 12, 4
FIT = OFF + (ROWS - 1) * LD + COLS          # 36: the last element the block owns is the tensor's last


def test_row_block_exact_fit_and_bounds():
    from avdino.ops import _rows
    t = torch.zeros(FIT)
    assert _rows(t, OFF, LD, ROWS, COLS, "blk") == t.data_ptr() + 4 * OFF
    assert _rows(t[:OFF + 2 * COLS], OFF, None, 2, COLS, "blk") == t.data_ptr() + 4 * OFF   # ld None: cols
    with pytest.raises(ValueError, match="blk bounds"):
        _rows(torch.zeros(FIT - 1), OFF, LD, ROWS, COLS, "blk")
    with pytest.raises(ValueError, match="blk"):
        _rows(t, -4, LD, ROWS, COLS, "blk")
    with pytest.raises(ValueError, match="blk"):
        _rows(torch.zeros(4 * FIT), OFF, COLS - 1, ROWS, COLS, "blk")
    with pytest.raises(ValueError, match="blk"):                 # one row: ld is still checked
        _rows(torch.zeros(4 * FIT), OFF, COLS - 1, 1, COLS, "blk")
    with pytest.raises(ValueError, match="blk bounds"):          # the second stride's extent counts
        _rows(t, OFF, LD, ROWS, COLS, "blk", extra=5)
    assert _rows(torch.zeros(FIT + 5), OFF, LD, ROWS, COLS, "blk", extra=5)


def test_row_block_alignment_dtype_and_contiguity():
    from avdino.ops import _rows
    t = torch.zeros(4 * FIT)
    assert _rows(t, OFF, LD, ROWS, COLS, "blk", align=4) == t.data_ptr() + 4 * OFF
    with pytest.raises(ValueError, match="multiples of 4"):
        _rows(t, 2, LD, ROWS, COLS, "blk", align=4)
    with pytest.raises(ValueError, match="multiples of 4"):
        _rows(t, OFF, 10, ROWS, COLS, "blk", align=4)
    assert _rows(t, 2, 10, ROWS, COLS, "blk") == t.data_ptr() + 4 * 2      # no alignment asked for
    h = torch.zeros(FIT, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="blk"):
        _rows(h, OFF, LD, ROWS, COLS, "blk")
    assert _rows(h, OFF, LD, ROWS, COLS, "blk", dtype=torch.bfloat16) == h.data_ptr() + 2 * OFF
    with pytest.raises(ValueError, match="blk"):
        _rows(torch.zeros(FIT), OFF, LD, ROWS, COLS, "blk", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="blk"):                 # a strided view of enough elements
        _rows(torch.zeros(2 * FIT)[::2], OFF, LD, ROWS, COLS, "blk")


def test_flat_checker():
    from avdino.ops import _flat
    t = torch.zeros(9)
    assert _flat(t, 9, "buf") == t.data_ptr()
    for bad in (None, t[:8], t.double(), torch.zeros(18)[::2]):
        with pytest.raises(ValueError, match="buf"):
            _flat(bad, 9, "buf")
    h = torch.zeros(9, dtype=torch.bfloat16)
    assert _flat(h, 9, "buf", torch.bfloat16) == h.data_ptr()


# ------------------------------------------------------------------ part two: recorded arguments
@pytest.fixture
def rec(monkeypatch):
    """ops.call records (name, *args) instead of calling (sizing queries with host outputs still
    run); ops.stream answers STREAM; the GEMM workspace is a CPU tensor (rec.ws)."""
    from avdino import ops
    real = ops.call

    class Rec(list):
        ws = torch.zeros(1 << 12)

        def only(self):
            assert len(self) == 1, self
            return self.pop()

    r = Rec()

    def call(name, *args):
        if name == "avd_lstm_ws":
            return real(name, *args)
        r.append((name,) + args)

    monkeypatch.setattr(ops, "call", call)
    monkeypatch.setattr(ops, "stream", lambda: STREAM)
    monkeypatch.setattr(ops, "_gemm_workspace", lambda device, n: r.ws)
    monkeypatch.setattr(ops, "TIMER", None)
    monkeypatch.setattr(ops, "SPANS", None)
    return r


def f32(n):
    return torch.zeros(n)


def bf16(n):
    return torch.zeros(n, dtype=torch.bfloat16)


def at(t, off=0):
    return t.data_ptr() + t.element_size() * off


def test_gate_arguments(rec):
    from avdino import ops
    from avdino._lib import lib
    rows, E = 4, 32
    cat, out, gi, ga = f32(8 + 3 * 72 + 64), f32(16 + 3 * 80 + 64), f32(1), f32(1)
    ops.gate_fwd(cat, gi, ga, out, rows, E, cat_ld=72, cat_off=8, out_ld=80, out_off=16)
    assert rec.only() == ("avd_gate_fwd", at(cat, 8), 72, at(gi), at(ga), at(out, 16), 80, 4, 32, STREAM)
    ops.gate_fwd(cat, gi, ga, out, rows, E)
    assert rec.only() == ("avd_gate_fwd", at(cat), 64, at(gi), at(ga), at(out), 64, 4, 32, STREAM)
    with pytest.raises(ValueError, match="cat"):
        ops.gate_fwd(cat[:-1], gi, ga, out, rows, E, cat_ld=72, cat_off=8)
    dout, dcat, dgi, dga = f32(3 * 68 + 64), f32(3 * 76 + 64), f32(1), f32(1)
    ws = f32(lib.avd_gate_bwd_ws(rows, E) + 3)
    ops.gate_bwd(dout, cat, gi, ga, dcat, dgi, dga, ws, rows, E, dout_ld=68, cat_ld=72, dcat_ld=76)
    assert rec.only() == ("avd_gate_bwd", at(dout), 68, at(cat), 72, at(gi), at(ga), at(dcat), 76, at(dgi),
                          at(dga), at(ws), ws.numel(), 4, 32, STREAM)
    with pytest.raises(ValueError, match="workspace"):
        ops.gate_bwd(dout, cat, gi, ga, dcat, dgi, dga, ws[:1], rows, E, dout_ld=68, cat_ld=72, dcat_ld=76)
    assert not rec


def test_layer_norm_arguments(rec):
    from avdino import ops
    from avdino._lib import lib
    rows, E = 3, 32
    x, res, y = f32(8 + 2 * 40 + 32), f32(2 * 36 + 32), f32(4 + 2 * 44 + 32)
    g, b, z, mean, rstd = f32(E), f32(E), f32(rows * E), f32(rows), f32(rows)
    so = torch.zeros(1, dtype=torch.int64)
    ops.ln_fwd(x, res, g, b, y, rows, E, z=z, mean=mean, rstd=rstd, eps=1e-6, drop_p=0.25, seed=7,
               seed_off=so, x_ld=40, x_off=8, res_ld=36, y_ld=44, y_off=4)
    assert rec.only() == ("avd_ln_fwd", at(x, 8), 40, at(res), 36, at(g), at(b), at(y, 4), 44, at(z), at(mean),
                          at(rstd), 3, 32, 1e-6, 0.25, 7, at(so), STREAM)
    ops.ln_fwd(x, None, g, b, y, rows, E)
    assert rec.only() == ("avd_ln_fwd", at(x), 32, None, 32, at(g), at(b), at(y), 32, None, None, None, 3, 32,
                          1e-5, 0.0, 0, None, STREAM)
    dy, dx, dr, dg, db = f32(4 + 2 * 40 + 32), f32(8 + 2 * 36 + 32), f32(2 * 48 + 32), f32(E), f32(E)
    ws = f32(lib.avd_ln_bwd_ws(rows, E) + 3)
    ops.ln_bwd(dy, z, mean, rstd, g, dx, dr, dg, db, ws, rows, E, drop_p=0.25, seed=7, seed_off=so,
               dy_ld=40, dy_off=4, dx_ld=36, dx_off=8, dr_ld=48)
    assert rec.only() == ("avd_ln_bwd", at(dy, 4), 40, at(z), at(mean), at(rstd), at(g), at(dx, 8), 36, at(dr), 48,
                          at(dg), at(db), at(ws), ws.numel(), 3, 32, 0.25, 7, at(so), STREAM)
    ops.ln_bwd(dy, z, mean, rstd, g, dx, None, dg, db, ws, rows, E)
    assert rec.only() == ("avd_ln_bwd", at(dy), 32, at(z), at(mean), at(rstd), at(g), at(dx), 32, None, 32,
                          at(dg), at(db), at(ws), ws.numel(), 3, 32, 0.0, 0, None, STREAM)
    with pytest.raises(ValueError, match="dx bounds"):
        ops.ln_bwd(dy, z, mean, rstd, g, dx, None, dg, db, ws, rows, E, dx_ld=36, dx_off=12)
    assert not rec


def test_mhsa_arguments(rec):
    from avdino import ops
    from avdino._lib import lib
    N, heads, T, dh = 2, 1, 5, 32
    E, R = heads * dh, N * T
    qkv, dqkv, ctx, dout, lse = f32(R * 3 * E), f32(R * 3 * E), f32(4 + (R - 1) * 36 + E), f32(R * E), f32(N * heads * T)
    so = torch.zeros(1, dtype=torch.int64)
    q, k, v = (qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E)
    ops.mhsa_fwd(q, k, v, (ctx, 4, 36), lse, N, heads, T, dh, 0.125, True, drop_p=0.5, seed=9, seed_off=so)
    assert rec.only() == ("avd_mhsa_fwd", at(qkv), 96, at(qkv, 32), 96, at(qkv, 64), 96, at(ctx, 4), 36, at(lse),
                          2, 1, 5, 32, 1, 0.125, 0.5, 9, at(so), STREAM)
    ops.mhsa_fwd(q, k, v, (ctx, 4, 36), None, N, heads, T, dh, 0.125, False)
    assert rec.only() == ("avd_mhsa_fwd", at(qkv), 96, at(qkv, 32), 96, at(qkv, 64), 96, at(ctx, 4), 36, None,
                          2, 1, 5, 32, 0, 0.125, 0.0, 0, None, STREAM)
    ws = f32(lib.avd_mhsa_bwd_ws(N, heads, T, dh) + 3)
    dq, dk, dv = (dqkv, 0, 3 * E), (dqkv, E, 3 * E), (dqkv, 2 * E, 3 * E)
    ops.mhsa_bwd((dout, 0, E), q, k, v, lse, dq, dk, dv, ws, N, heads, T, dh, 0.125, False, drop_p=0.5, seed=9,
                 seed_off=so)
    assert rec.only() == ("avd_mhsa_bwd", at(dout), 32, at(qkv), 96, at(qkv, 32), 96, at(qkv, 64), 96, at(lse),
                          at(dqkv), 96, at(dqkv, 32), 96, at(dqkv, 64), 96, at(ws), ws.numel(), 2, 1, 5, 32, 0,
                          0.125, 0.5, 9, at(so), STREAM)
    with pytest.raises(ValueError, match="dv bounds"):
        ops.mhsa_bwd((dout, 0, E), q, k, v, lse, dq, dk, (dqkv[:-1], 2 * E, 3 * E), ws, N, heads, T, dh, 0.125, False)
    assert not rec


def test_xattn_arguments(rec):
    from avdino import ops
    from avdino._lib import lib
    dirs, groups, B, E = 2, 2, 2, 32
    rows = groups * B
    ds = rows * 3 * E                                           # one direction's [rows, 3E] projections
    qkv, dqkv = f32(dirs * ds), f32(dirs * ds)
    x, out, dout, lse = f32(rows * 2 * E), f32(rows * 2 * E), f32(rows * 2 * E), f32(dirs * rows)
    q, k, v = (qkv, 0, 3 * E, ds), (qkv, E, 3 * E, ds), (qkv, 2 * E, 3 * E, ds)
    ops.xattn_fwd(q, k, v, (x, 0, 2 * E, E), (out, 0, 2 * E, E), lse, dirs, groups, B, E, 0.25)
    assert rec.only() == ("avd_xattn_fwd", at(qkv), 96, 384, at(qkv, 32), 96, 384, at(qkv, 64), 96, 384,
                          at(x), 64, 32, at(out), 64, 32, at(lse), 2, 2, 2, 32, 0.25, STREAM)
    ops.xattn_fwd(q, k, v, (x, 0, 2 * E, E), (out, 0, 2 * E, E), None, dirs, groups, B, E, 0.25)
    assert rec.only()[16] is None
    ws = f32(lib.avd_xattn_bwd_ws(dirs, groups, B, E) + 3)
    dq, dk, dv = (dqkv, 0, 3 * E, ds), (dqkv, E, 3 * E, ds), (dqkv, 2 * E, 3 * E, ds)
    ops.xattn_bwd((dout, 0, 2 * E, E), q, k, v, lse, dq, dk, dv, ws, dirs, groups, B, E, 0.25)
    assert rec.only() == ("avd_xattn_bwd", at(dout), 64, 32, at(qkv), 96, 384, at(qkv, 32), 96, 384,
                          at(qkv, 64), 96, 384, at(lse), at(dqkv), 96, 384, at(dqkv, 32), 96, 384,
                          at(dqkv, 64), 96, 384, at(ws), ws.numel(), 2, 2, 2, 32, 0.25, STREAM)
    with pytest.raises(ValueError, match="dv bounds"):          # the second direction falls off the end
        ops.xattn_bwd((dout, 0, 2 * E, E), q, k, v, lse, dq, dk, (dqkv[:-1], 2 * E, 3 * E, ds), ws, dirs, groups,
                      B, E, 0.25)
    with pytest.raises(ValueError, match="multiple"):           # direction stride not a multiple of 4
        ops.xattn_fwd(q, k, v, (x, 0, 2 * E, E - 2), (out, 0, 2 * E, E), lse, dirs, groups, B, E, 0.25)
    assert not rec


def test_softmax_rows_arguments(rec):
    from avdino import ops
    R, C = 3, 5
    s, pr, dp = f32(2 * 8 + C), f32(2 * 8 + C), f32(2 * 12 + C)
    ops.softmax_rows_fwd(s, R, C, ld=8)
    assert rec.only() == ("avd_softmax_rows_fwd", at(s), 8, 3, 5, STREAM)
    ops.softmax_rows_bwd(pr, dp, R, C, ldp=8, lddp=12)
    assert rec.only() == ("avd_softmax_rows_bwd", at(pr), 8, at(dp), 12, 3, 5, STREAM)
    for bad in (lambda: ops.softmax_rows_fwd(s[:-1], R, C, ld=8), lambda: ops.softmax_rows_fwd(s, R, C, ld=4),
                lambda: ops.softmax_rows_bwd(pr, dp[:-1], R, C, ldp=8, lddp=12),
                lambda: ops.softmax_rows_bwd(pr, dp, 0, C, ldp=8, lddp=12)):
        with pytest.raises(ValueError, match="softmax rows"):
            bad()
    assert not rec


def test_lstm_arguments(rec):
    from avdino import ops
    N, T, H = 1, 5, 16
    ns, ng = N * T * 2 * 6 * H, N * T * 2 * 4 * H               # avd_lstm_ws: act + hprev, and gx / dg
    assert ops.lstm_ws(N, T, H) == (ns, ng)
    gx, wf, wr, out, save, dg = f32(ng), f32(4 * H * H), f32(4 * H * H), f32(N * 2 * H), f32(ns), f32(ng)
    ops.lstm_fwd(gx, wf, wr, out, save, N, T, H, True)
    assert rec.only() == ("avd_lstm_fwd", at(gx), at(wf), at(wr), at(out), at(save), 1, 1, 1, 5, 16, STREAM)
    ops.lstm_fwd(gx, wf, wr, out, None, N, T, H, False)
    assert rec.only() == ("avd_lstm_fwd", at(gx), at(wf), at(wr), at(out), None, 0, 0, 1, 5, 16, STREAM)
    ops.lstm_bwd(out, wf, wr, save, dg, N, T, H, True)
    assert rec.only() == ("avd_lstm_bwd", at(out), at(wf), at(wr), at(save), at(dg), 1, 1, 5, 16, STREAM)


def test_xent_fused_arguments(rec):
    from avdino import ops
    from avdino._lib import lib
    R, C, P = 4, 6, 128
    q, k, dq, dk, loss = f32(R * P), f32(C * P), f32(R * P), f32(C * P), f32(R)
    ws = f32(lib.avd_xent_fused_ws(R, C, P) + 5)
    ops.xent_fused(q, k, R, C, P, 2, (0, 2), (-1, 3), 10.0, 0.5, loss, dq, dk, ws)
    assert rec.only() == ("avd_xent_fused", at(q), at(k), 4, 6, 128, 2, 0, 2, -1, 3, 10.0, 0.5, at(loss), at(dq),
                          at(dk), at(ws), ws.numel(), STREAM)
    for bad in (dict(k=k[:-1]), dict(loss=loss.double()), dict(dq=torch.zeros(2 * R * P)[::2])):
        a = dict(q=q, k=k, loss=loss, dq=dq, dk=dk)
        a.update(bad)
        with pytest.raises(ValueError, match="xent operand"):
            ops.xent_fused(a["q"], a["k"], R, C, P, 2, (0, 2), (-1, 3), 10.0, 0.5, a["loss"], a["dq"], a["dk"], ws)
    with pytest.raises(ValueError, match="xent workspace"):
        ops.xent_fused(q, k, R, C, P, 2, (0, 2), (-1, 3), 10.0, 0.5, loss, dq, dk, ws[:8])
    assert not rec


def test_linear_bwd_arguments(rec):
    """Both paired branches of linear_bwd: dW + dX (which = 3) and dW alone (which = 1: no W, no
    dX, dx_ld = In)."""
    from avdino import ops
    from avdino._lib import lib
    rows, O, In = 3, 8, 16
    dout, x, dx = f32(4 + 2 * 12 + O), f32(4 + 2 * 20 + In), f32(8 + 2 * 24 + In)
    w, dw, db = torch.zeros(O, In), torch.zeros(O, In), f32(O)
    for mode in (ops.GEMM_F32_MFMA, ops.GEMM_BF16_MFMA):
        nws = lib.avd_linear_bwd_ws_elems(rows, O, In, mode)
        ops.linear_bwd(dout, x, w, dw, db, dx, rows, dout_ld=12, dout_off=4, x_ld=20, x_off=4, dx_ld=24,
                       dx_off=8, mode=mode)
        assert rec.only() == ("avd_linear_bwd", 3, 8, 16, at(dout, 4), 12, at(x, 4), 20, at(w), at(dw), at(dx, 8),
                              24, at(db), mode, 3, at(rec.ws), nws, STREAM)
        ops.linear_bwd(dout, x, w, dw, None, None, rows, dout_ld=12, dout_off=4, x_ld=20, x_off=4, dx_ld=24,
                       mode=mode)
        assert rec.only() == ("avd_linear_bwd", 3, 8, 16, at(dout, 4), 12, at(x, 4), 20, None, at(dw), None, 16,
                              None, mode, 1, at(rec.ws), nws, STREAM)
    for bad in (dict(dout_off=8), dict(x_ld=21), dict(dx_off=12)):
        a = dict(dout_ld=12, dout_off=4, x_ld=20, x_off=4, dx_ld=24, dx_off=8)
        a.update(bad)
        with pytest.raises(ValueError, match="linear_bwd"):
            ops.linear_bwd(dout, x, w, dw, db, dx, rows, **a)
    assert not rec


def test_linear_hwc_arguments(rec):
    from avdino import ops
    from avdino._lib import lib
    rows, O, C, HW = 3, 8, 8, 4
    In = C * HW
    nws = lib.avd_linear_hwc_ws_elems(rows, O, In)
    feat, wp, dxh = bf16(rows * In), bf16(O * In), bf16(rows * In)
    b, out, dout, dw, db = f32(O), f32(8 + 2 * 20 + O), f32(8 + 2 * 20 + O), f32(O * In), f32(O)
    ops.linear_fwd_hwc(feat, wp, b, out, rows, O, C, HW, out_ld=20, out_off=8)
    assert rec.only() == ("avd_linear_fwd_hwc", 3, 8, 8, 4, at(feat), at(wp), at(b), at(out, 8), 20, at(rec.ws),
                          nws, STREAM)
    ops.linear_bwd_hwc(dout, feat, wp, dw, db, dxh, rows, O, C, HW, dout_ld=20, dout_off=8)
    assert rec.only() == ("avd_linear_bwd_hwc", 3, 8, 8, 4, at(dout, 8), 20, at(feat), at(wp), at(dw), at(db),
                          at(dxh), 3, at(rec.ws), nws, STREAM)
    ops.linear_bwd_hwc(dout, feat, wp, dw, None, dxh, rows, O, C, HW, which=1)
    assert rec.only() == ("avd_linear_bwd_hwc", 3, 8, 8, 4, at(dout), 8, at(feat), at(wp), at(dw), None, at(dxh),
                          1, at(rec.ws), nws, STREAM)
    with pytest.raises(ValueError, match="hwc fwd out"):
        ops.linear_fwd_hwc(feat, wp, b, out[:-1], rows, O, C, HW, out_ld=20, out_off=8)
    with pytest.raises(ValueError, match="hwc bwd dout"):
        ops.linear_bwd_hwc(dout, feat, wp, dw, db, dxh, rows, O, C, HW, dout_ld=20, dout_off=12)
    with pytest.raises(ValueError, match="hwc bwd dX"):
        ops.linear_bwd_hwc(dout, feat, wp, dw, db, dxh.float(), rows, O, C, HW)
    assert not rec
