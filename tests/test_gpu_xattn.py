"""avd_xattn_fwd / avd_xattn_bwd (csrc/xattn.hip), the gate ops and the plain route's row softmax
against float64 written out here (and held to torch CPU autograd at 1e-12).

Tiling named for the shapes below: a block owns XQ = 64 query rows (backward column pass: 64
keys) and streams the other side in XB = 32-row tiles, so B = 130 spans 3 query tiles and 5 key
tiles with a ragged last one of each; B = 16 / 17 / 64 / 80 sit on and next to the 16-row wave
and the tile edges.

Band of the bf16 kernel (computed, per output tensor, rel-L2): the same formulas in float64 with
Q, K, V, dO rounded to bf16 and P (and dS) rounded to bf16 before the second product -- the
kernel's roundings, with P below the smallest normal f32 zero as the hardware exponential gives
it -- against unrounded float64, times 3 (f32 accumulation order, exp).  The measured error is
printed beside the bound (run with -s).

The same band is applied per slice of the 2-D outputs (out, dq, dk, dv): every 16-column feature
tile over all rows (an MFMA accumulator, a feature chunk of the backward), and every 16-row tile
of every group over all columns (a wave's ownership).  A whole-tensor rel-L2 dilutes a wrong tile
by the square root of the tile count; a slice does not.  Slices whose exact value or whose model
error is exactly zero are skipped (the B = 1 gradients, covered by the zero branch).  SLICE_F is
the project's factor 3; the largest err / model ratio over every slice of every case is printed
per tensor (MEASURED below).

E runs over ops.XATTN_DIMS: 64 is the one size with a single 64-column chunk and one staging
task per thread; 256 (configs/config_multimodal_dino.yaml) is the one whose staging loads four
tasks per thread together, fully unrolled, and the smallest whose backward is cut in feature
chunks (grid z = 2); 512 stages rolled, one task at a time.

At B = 17 the planted row 16 is alone in its row tile and its softmax is one-hot to float64, so
its exact dQ is ~e^-100 of a typical row's: the reference writes dS in the form that keeps such a
row right (reference()), and the kernel has to as well (before it kept delta relative to the top
key's dP, these slices came out ~1e-6 of a typical row, 1e34 to 1e42 x the model).

MEASURED on an MI355X, largest slice err / model ratio over all 70 cases: out 1.373 (g1 B130 E32,
rows 128..129), dq 1.008, dk 1.003, dv 1.004.
"""
import math

import pytest
import torch

from avdino import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 777.0
XQ, XB = 64, 32
TILE = 16                            # MFMA tile: feature columns of an accumulator, rows of a wave
SLICE_F = 3.0                        # slice band factor (module docstring)
DIMS = ops.XATTN_DIMS                # every dispatched E (tests/test_dispatch_tables_cpu.py)
BS = (1, 5, 16, 17, 64, 80, 130)
GROUPS = (1, 3)
TWO_DIR_DIMS = (32, 256)


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def make_inputs(groups, B, E, seed):
    """f32 Q, K, V, X, dO [groups, B, E]: logits scale Q K^T of std ~8, planted rows with
    |logit| > 100 whose maximum sits in the last / the first key tile, per-group V scales."""
    g = torch.Generator().manual_seed(seed)
    scale = E ** -0.5
    q = torch.randn(groups, B, E, generator=g) * math.sqrt(8.0)
    k = torch.randn(groups, B, E, generator=g) * math.sqrt(8.0)
    v = torch.randn(groups, B, E, generator=g)
    x = torch.randn(groups, B, E, generator=g)
    do = torch.randn(groups, B, E, generator=g)
    for gi in range(groups):
        v[gi] *= 10.0 ** gi                        # leakage between groups shows at once
        if B >= 2:
            # row 0 -> key B - 1 (last key tile), row B - 1 -> key 0 (first), logit ~ +-120
            for row, key, sign in ((0, B - 1, 1.0), (B - 1, 0, 1.0), (B // 2, B - 1, -1.0)):
                kk = k[gi, key]
                q[gi, row] = sign * kk * (120.0 / (scale * float(kk @ kk)))
    return q, k, v, x, do, scale


def autograd_reference(q, k, v, x, do, scale):
    """float64 OUT, LSE, dQ, dK, dV by torch autograd (exact to 1e-16 of each tensor's scale)."""
    q, k, v, x, do = (t.to(torch.float64) for t in (q, k, v, x, do))
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = scale * q @ k.transpose(1, 2)
    out = x + s.softmax(-1) @ v
    out.backward(do)
    return (out.detach(), torch.logsumexp(s.detach(), -1), q.grad, k.grad, v.grad)


def reference(q, k, v, x, do, scale, rounded):
    """float64 OUT, LSE, dQ, dK, dV; rounded=True applies the kernel's bf16 roundings.

    dS = P o (dP - delta) is written as dS_ij = P_ij sum_l P_il (dP_ij - dP_il): in a row whose
    softmax is one-hot to float64 (the planted rows) dP_top - sum_l P_il dP_il is zero by rounding
    while the true value is sum_l P_il (dP_top - dP_l) ~ e^-100 |dP|; a slice that holds only such
    a row (B = 17: row 16 alone in its tile) needs the reference right at that scale."""
    q, k, v, x, do = (t.to(torch.float64) for t in (q, k, v, x, do))
    if rounded:
        q, k, v, do = bf(q), bf(k), bf(v), bf(do)
    s = scale * q @ k.transpose(1, 2)
    p = s.softmax(-1)
    if rounded:
        # the kernel's P is an f32 from the hardware exponential, which has no subnormals: below
        # 2^-126 it is zero (the whole dQ of a planted row of g2, V x 100, comes from such P)
        p = torch.where(p < 2.0 ** -126, torch.zeros_like(p), p)
    dp = do @ v.transpose(1, 2)
    ds = p * ((dp.unsqueeze(-1) - dp.unsqueeze(-2)) * p.unsqueeze(-2)).sum(-1)
    pr = p
    if rounded:
        pr, ds = bf(p), bf(ds)
    return (x + pr @ v, torch.logsumexp(s, -1), scale * ds @ k, scale * ds.transpose(1, 2) @ q,
            pr.transpose(1, 2) @ do)


def rel(a, ref):
    return float((a - ref).norm() / ref.norm())


def slice_ratios(t, ex, mo):
    """err / model-err ratios of [groups, B, E] tensors over every 16-column feature tile (all
    rows) and every 16-row tile of every group (all columns); slices with a zero exact value or a
    zero model error are left out.  -> (largest ratio, its slice with |exact|, the model's and the
    kernel's error there, number of slices checked)."""
    worst, where, n = 0.0, None, 0
    groups, B, E = ex.shape
    slices = [("cols", c0, (slice(None), slice(None), slice(c0, c0 + TILE))) for c0 in range(0, E, TILE)]
    slices += [(f"g{gi} rows", r0, (gi, slice(r0, min(B, r0 + TILE)), slice(None)))
               for gi in range(groups) for r0 in range(0, B, TILE)]
    for kind, at, ix in slices:
        e = ex[ix]
        den, merr = float(e.norm()), float((mo[ix] - e).norm())
        if den == 0.0 or merr == 0.0:
            continue
        n += 1
        err = float((t[ix] - e).norm())
        ratio = err / merr
        if ratio > worst:
            worst, where = ratio, f"{kind} {at} (|exact| {den:.2e}, model err {merr:.2e}, err {err:.2e})"
    return worst, where, n


def run_kernel(q, k, v, x, do, scale, groups, B, E):
    """Q / K / V as column slices of a [rows, 3E] buffer, X / OUT as halves of [rows + 2, 2E]
    buffers, the gradients as slices of a [rows + 1, 4E] buffer; everything else sentinel."""
    from avdino import ops
    rows = groups * B
    qkv = torch.cat([q, k, v], -1).reshape(rows, 3 * E).contiguous().to(DEV)
    xb = torch.full((rows + 2, 2 * E), SENT)
    xb[:rows, E:] = x.reshape(rows, E)
    xb = xb.to(DEV)
    ob = torch.full((rows + 2, 2 * E), SENT, device=DEV)
    lse = torch.full((rows + 3,), SENT, device=DEV)
    ops.xattn_fwd((qkv, 0, 3 * E, 0), (qkv, E, 3 * E, 0), (qkv, 2 * E, 3 * E, 0), (xb, E, 2 * E, 0),
                  (ob, 0, 2 * E, 0), lse, 1, groups, B, E, scale)
    dob = torch.full((rows + 2, 2 * E), SENT)
    dob[:rows, :E] = do.reshape(rows, E)
    dob = dob.to(DEV)
    gb = torch.full((rows + 1, 4 * E), SENT, device=DEV)
    ws = torch.empty(ops.xattn_bwd_ws(1, groups, B, E), device=DEV)
    ops.xattn_bwd((dob, 0, 2 * E, 0), (qkv, 0, 3 * E, 0), (qkv, E, 3 * E, 0), (qkv, 2 * E, 3 * E, 0), lse,
                  (gb, 0, 4 * E, 0), (gb, E, 4 * E, 0), (gb, 3 * E, 4 * E, 0), ws, 1, groups, B, E, scale)
    torch.cuda.synchronize()
    return ob.cpu(), lse.cpu(), gb.cpu()


@pytest.mark.parametrize("E", DIMS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("groups", GROUPS)
def test_xattn_matches_float64(groups, B, E):
    q, k, v, x, do, scale = make_inputs(groups, B, E, 1000 * groups + 10 * B + E)
    rows = groups * B
    if B >= 2:
        s = scale * q.double() @ k.double().transpose(1, 2)
        assert 4.0 < float(s.std()) and float(s.abs().max()) > 100.0     # the inputs do their job
        if B > XB:
            assert int(s[0, 0].argmax()) >= (B - 1) // XB * XB and int(s[0, B - 1].argmax()) < XB
    exact = reference(q, k, v, x, do, scale, rounded=False)
    model = reference(q, k, v, x, do, scale, rounded=True)
    for name, ex, ag in zip(("out", "lse", "dq", "dk", "dv"), exact, autograd_reference(q, k, v, x, do, scale)):
        assert float((ex - ag).norm()) <= 1e-12 * float(ag.norm()), name      # the formulas written out
    ob, lse, gb = run_kernel(q, k, v, x, do, scale, groups, B, E)
    ob2, lse2, gb2 = run_kernel(q, k, v, x, do, scale, groups, B, E)
    assert torch.equal(ob, ob2) and torch.equal(lse, lse2) and torch.equal(gb, gb2), "not bit-reproducible"
    # nothing outside the owned rows / columns is written
    assert bool((ob[:rows, E:] == SENT).all()) and bool((ob[rows:] == SENT).all())
    assert bool((lse[rows:] == SENT).all())
    assert bool((gb[rows:] == SENT).all()) and bool((gb[:rows, 2 * E:3 * E] == SENT).all())
    got = (ob[:rows, :E], lse[:rows], gb[:rows, :E], gb[:rows, E:2 * E], gb[:rows, 3 * E:])
    names = ("out", "lse", "dq", "dk", "dv")
    for name, t, ex, mo in zip(names, got, exact, model):
        t = t.double().reshape(ex.shape)
        assert bool(torch.isfinite(t).all()), name
        if float(ex.norm()) == 0.0:
            # B = 1: a one-key softmax has no gradient to its logit, dQ = dK = 0 exactly.  The
            # kernel forms p (dP - delta) from two f32 MFMA sums of the same E products in
            # different operand roles: zero up to their accumulation noise, E 2^-24 relative
            dp = float((do.double() * v.double()).sum(-1).abs().max())
            lim = 1e-4 * scale * dp * float(max(q.abs().max(), k.abs().max()))
            print(f"xattn g{groups} B{B} E{E} {name}: max |.| {float(t.abs().max()):.2e} (limit {lim:.2e})")
            assert float(t.abs().max()) <= lim, name
            continue
        err, bound = rel(t, ex), 3.0 * rel(mo, ex)
        print(f"xattn g{groups} B{B} E{E} {name}: rel-L2 {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (name, err, bound)
        if t.dim() == 3:
            worst, where, n = slice_ratios(t, ex, mo)
            print(f"xattn g{groups} B{B} E{E} {name}: slice err/model max {worst:.3f} of {n} slices at {where}")
            assert worst <= SLICE_F, (name, where, worst)


@pytest.mark.parametrize("E", TWO_DIR_DIMS)
def test_xattn_two_directions_one_launch(E):
    """dirs = 2 in the engine's layout: projections [2][rows][3E], X / OUT / dOUT the halves of
    [rows, 2E] buffers (direction stride E)."""
    from avdino import ops
    groups, B = 3, 17
    rows = groups * B
    ins = [make_inputs(groups, B, E, 40 + d) for d in range(2)]
    scale = ins[0][5]
    qkv = torch.stack([torch.cat(i[:3], -1).reshape(rows, 3 * E) for i in ins]).contiguous().to(DEV)
    xb = torch.cat([i[3].reshape(rows, E) for i in ins], 1).contiguous().to(DEV)
    dob = torch.cat([i[4].reshape(rows, E) for i in ins], 1).contiguous().to(DEV)
    ob = torch.full((rows, 2 * E), SENT, device=DEV)
    lse = torch.empty(2 * rows, device=DEV)
    ds = rows * 3 * E
    ops.xattn_fwd((qkv, 0, 3 * E, ds), (qkv, E, 3 * E, ds), (qkv, 2 * E, 3 * E, ds), (xb, 0, 2 * E, E),
                  (ob, 0, 2 * E, E), lse, 2, groups, B, E, scale)
    gb = torch.full((2, rows, 3 * E), SENT, device=DEV)
    ws = torch.empty(ops.xattn_bwd_ws(2, groups, B, E), device=DEV)
    ops.xattn_bwd((dob, 0, 2 * E, E), (qkv, 0, 3 * E, ds), (qkv, E, 3 * E, ds), (qkv, 2 * E, 3 * E, ds), lse,
                  (gb, 0, 3 * E, ds), (gb, E, 3 * E, ds), (gb, 2 * E, 3 * E, ds), ws, 2, groups, B, E, scale)
    ob, gb, lse = ob.cpu().double(), gb.cpu().double(), lse.cpu().double()
    for d, i in enumerate(ins):
        exact = reference(*i[:5], scale, rounded=False)
        model = reference(*i[:5], scale, rounded=True)
        got = (ob[:, d * E:(d + 1) * E], lse[d * rows:(d + 1) * rows], gb[d, :, :E], gb[d, :, E:2 * E],
               gb[d, :, 2 * E:])
        for name, t, ex, mo in zip(("out", "lse", "dq", "dk", "dv"), got, exact, model):
            err, bound = rel(t.reshape(ex.shape), ex), 3.0 * rel(mo, ex)
            print(f"xattn dir{d} E{E} {name}: rel-L2 {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (d, name, err, bound)


def test_xattn_null_lse():
    """The teacher / eval passes give no lse: same OUT."""
    from avdino import ops
    groups, B, E = 2, 80, 128
    q, k, v, x, _do, scale = make_inputs(groups, B, E, 5)
    rows = groups * B
    t = [a.reshape(rows, E).contiguous().to(DEV) for a in (q, k, v, x)]
    o1, o2 = torch.empty(rows, E, device=DEV), torch.empty(rows, E, device=DEV)
    lse = torch.empty(rows, device=DEV)
    ms = [(a, 0, E, 0) for a in t]
    ops.xattn_fwd(*ms, (o1, 0, E, 0), lse, 1, groups, B, E, scale)
    ops.xattn_fwd(*ms, (o2, 0, E, 0), None, 1, groups, B, E, scale)
    assert torch.equal(o1, o2)


# ---------------------------------------------------------------- gates
@pytest.mark.parametrize("E", [32, 256])
@pytest.mark.parametrize("rows", [1, 7, 300])
def test_gate_ops_match_float64(rows, E):
    from avdino import ops
    g = torch.Generator().manual_seed(rows + E)
    cat = torch.randn(rows, 2 * E, generator=g)
    dout = torch.randn(rows, 2 * E, generator=g)
    gi, ga = torch.tensor(0.3), torch.tensor(-0.8)
    c64 = cat.double()
    gi64, ga64 = gi.double().requires_grad_(True), ga.double().requires_grad_(True)
    c64.requires_grad_(True)
    out = torch.cat([torch.sigmoid(gi64) * c64[:, :E], torch.sigmoid(ga64) * c64[:, E:]], 1)
    out.backward(dout.double())
    dcat, dgi, dga = (torch.empty(rows, 2 * E, device=DEV), torch.empty((), device=DEV),
                      torch.empty((), device=DEV))
    o = torch.empty(rows, 2 * E, device=DEV)
    catd, doutd, gid, gad = cat.to(DEV), dout.to(DEV), gi.to(DEV), ga.to(DEV)
    ops.gate_fwd(catd, gid, gad, o, rows, E)
    ws = torch.empty(ops.gate_bwd_ws(rows, E), device=DEV)
    runs = []
    for _ in range(2):
        ops.gate_bwd(doutd, catd, gid, gad, dcat, dgi, dga, ws, rows, E)
        runs.append((dcat.cpu().clone(), dgi.cpu().clone(), dga.cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "gate gradients not bit-reproducible"
    # elementwise f32 products: a few ulp (6e-8 each)
    assert rel(o.cpu().double(), out.detach()) < 1e-6
    assert rel(runs[0][0].double(), c64.grad) < 1e-6
    # the scalar gradients are f32 sums of rows * E products t_i: error << 1e-5 sum |t_i| (the
    # worst case of any summation order is n 2^-24 sum |t_i|, n <= 76800, i.e. 4.6e-3 sum |t_i|;
    # partial sums of <= 64 terms and trees stay orders below); a swapped or missing half is off
    # by the sum itself
    tol = 1e-5 * float(dout.double().mul(c64.detach()).abs().sum())
    for got, ref in ((runs[0][1], gi64.grad), (runs[0][2], ga64.grad)):
        assert float(ref) != 0.0 and abs(float(got) - float(ref)) <= tol, (float(got), float(ref), tol)


# ---------------------------------------------------------------- plain-route row softmax
@pytest.mark.parametrize("R,C", [(1, 1), (5, 5), (70, 130)])
def test_softmax_rows_match_float64(R, C):
    from avdino import ops
    g = torch.Generator().manual_seed(R * C)
    s = torch.randn(R, C, generator=g) * 8.0
    dp = torch.randn(R, C, generator=g)
    s64 = s.double().requires_grad_(True)
    p64 = s64.softmax(-1)
    p64.backward(dp.double())
    sd, dpd = s.to(DEV), dp.to(DEV)
    ops.softmax_rows_fwd(sd, R, C)
    ops.softmax_rows_bwd(sd, dpd, R, C)
    assert float((sd.cpu().double() - p64.detach()).abs().max()) < 1e-6
    assert float((dpd.cpu().double() - s64.grad).abs().max()) < 1e-5
