"""The fused layer backward's second shape, the audio conv3 (28x28, 16 -> 32, 5x5 pad 2;
avd_cl_layer_bwd / avd_cl_layer_bwd_codes, csrc/lbwd.hip LbA3), against the three launches it
replaces -- avd_cl_bn_bwd_apply, avd_cl_conv_dgrad (DgrA3) and avd_cl_conv_wgrad (WgA3) -- on
the same bf16 operands (test_gpu_lbwd_codes.py's: negative scales, exact in-window ties, windows
whose BN output is <= 0 everywhere, zero pooled gradients):

* dX: the kernel keeps DgrA3's k order (k-step = one tap x 32 dY channels), so it is bit-identical
  to the separate input gradient; dW (f32 slabs summed by avd_sum_rows, another slab partition)
  within 1e-6 rel-L2 of the separate weight gradient;
* the three apply variants -- dY handed in, relu(bn(y)) recomputed per window, the pooled
  gradient routed by the forward pool's code words (scale / shift NaN: it reads neither) -- give
  the same dX and summed dW bit for bit at the same slab count;
* at N <= 12 against float64 of the same dY: dX rel-L2 < 5e-3 (its bf16 store), dW < 1e-5;
* dX and the slabs are pre-filled with NaN and written everywhere, and the sentinel past the end
  of both buffers is untouched;
* 28x20, 20x28 and 28^2 with other channel counts are declined: the slab query answers 0, a
  launch returns AVD_ERR_SHAPE and writes nothing;
* an engine step with ConvBranch.LAYER_BWD_28 on equals the step with it off (loss, every
  gradient not fed by this layer bit for bit, conv3.weight within 1e-6, the tensors fed by its
  dX within 1e-3), and LAYER_BWD_CODES on equals off bit for bit.

(N, B, grid cap): a single sample split between two blocks (1, 1, 2); blocks that start
mid-sample, continuation tiles and BN-group changes inside a block's range (12, 4, 5); one or
few tiles per block (10, 5); APPLY_GMAX = 8 groups (8, 1, 3); an uncapped grid with more tiles
than blocks (512, 64: 3584 tiles)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = torch.bfloat16
F64 = torch.float64
CIN, COUT, K, PAD, H = 16, 32, 5, 2, 28
HP = H // 2
NW = COUT * CIN * K * K
AVD_ERR_SHAPE = -1
TAIL, SENT = 4096, 777.0

CASES = [(1, 1, 2), (12, 4, 5), (10, 5, None), (8, 1, 3), (512, 64, None)]
IDS = ["single_sample", "capped", "few_tiles_per_block", "gmax_groups", "uncapped"]


@functools.lru_cache(maxsize=None)
def _operands(N, B):
    g = torch.Generator(device="cuda").manual_seed(280 + N)
    G = N // B

    def r(*s, lo=-1.0, hi=1.0):
        return torch.rand(*s, generator=g, device="cuda") * (hi - lo) + lo

    def mask(p):
        return torch.rand(N, HP, HP, COUT, generator=g, device="cuda") < p
    y = r(N, H, H, COUT, lo=-2, hi=2).to(T)
    gout = (r(N, HP, HP, COUT) * 1e-3).to(T)
    x = r(N, H, H, CIN, lo=0, hi=2).to(T)
    scale, shift = r(G * COUT, lo=0.5, hi=1.5), r(G * COUT, lo=-0.5, hi=0.5)
    scale[1::3] *= -1.0                                   # negative scales: the max is y's min
    coef = torch.stack([r(G * COUT, lo=0.5, hi=1.5), r(G * COUT) * 1e-3, r(G * COUT) * 1e-4], 1).contiguous()
    w = r(COUT, CIN, K, K) * 0.1
    # exact ties inside a window (views of y: window pixel (i, j) over all windows)
    p00, p01, p10, p11 = y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2]
    m = mask(0.2)
    p01[m] = p00[m]
    m = mask(0.1)
    p11[m] = p10[m]
    m = mask(0.1)
    p10[m] = p00[m]
    m = mask(0.05)
    for q in (p01, p10, p11):
        q[m] = p00[m]
    # windows with BN output <= 0 at all four pixels: |scale| * 2 >= 1 > shift
    dead = mask(0.15)
    neg = (-2.0 * torch.sign(scale)).view(G, 1, 1, 1, COUT).expand(G, B, HP, HP, COUT).reshape(N, HP, HP, COUT).to(T)
    for q in (p00, p01, p10, p11):
        q[dead] = neg[dead]
    gout[mask(0.2)] = 0
    return y, gout, x, scale, shift, coef.view(-1), w


def _padded(numel, dtype):
    """numel NaNs followed by TAIL sentinels: (the whole buffer, the NaN part)."""
    full = torch.full((numel + TAIL,), SENT, device="cuda", dtype=dtype)
    full[:numel] = float("nan")
    return full, full[:numel]


def _tail_ok(full, numel):
    return bool((full[numel:] == SENT).all())


def _reference(ops, y, gout, x, scale, shift, coef, wk_d, N, B):
    dy = torch.empty_like(y)
    ops.cl_bn_bwd_apply(y, gout, 0, scale, shift, coef, dy, N, B, COUT, H, H)
    dx = torch.empty(N, H, H, CIN, dtype=T, device="cuda")
    ops.cl_conv_dgrad(dy, wk_d, dx, N, CIN, H, H, COUT, K, PAD)
    nch = ops.cl_wgrad_chunks(N, COUT, CIN, K)
    parts = torch.empty(nch * NW, device="cuda")
    ops.cl_conv_wgrad(x, dy, parts, N, CIN, H, H, COUT, K, PAD)
    dw = torch.empty(NW, device="cuda")
    ops.sum_rows(parts, nch, NW, dw)
    return dy, dx, dw


def _fused(ops, y, gout, x, scale, shift, coef, dy, wk_d, N, B, slabs, codes=None):
    pfull, parts = _padded(slabs * NW, torch.float32)
    dfull, dx = _padded(N * H * H * CIN, T)
    ops.cl_layer_bwd(y, gout, scale, shift, coef, dy, x, wk_d, dx, parts, slabs, N, B, CIN, H, H, COUT, K,
                     PAD, codes=codes)
    dw = torch.empty(NW, device="cuda")
    ops.sum_rows(parts, slabs, NW, dw)
    torch.cuda.synchronize()
    # every element written, nothing past the ends
    assert not bool(torch.isnan(dx).any()) and not bool(torch.isnan(parts).any())
    assert _tail_ok(dfull, dx.numel()) and _tail_ok(pfull, parts.numel())
    return dx.view(N, H, H, CIN), dw


def _wgrad64(x, dy):
    xp = torch.nn.functional.pad(x.to(F64), (0, 0, PAD, PAD, PAD, PAD))
    d = dy.to(F64).reshape(-1, COUT)
    dw = torch.zeros(COUT, CIN, K, K, dtype=F64, device="cuda")
    for i in range(K):
        for j in range(K):
            dw[:, :, i, j] = d.T @ xp[:, i:i + H, j:j + H, :].reshape(-1, CIN)
    return dw.reshape(-1)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("N,B,cap", CASES, ids=IDS)
def test_layer_bwd28_equals_apply_dgrad_wgrad(N, B, cap, avd_opts, capsys):
    from avdino import ops
    if cap:
        avd_opts(grid_cap=cap)
    y, gout, x, scale, shift, coef, w = _operands(N, B)
    wk_d = torch.empty(ops.cl_weight_elems(COUT, CIN, K, 1), dtype=T, device="cuda")
    ops.cl_weight_layout(w, wk_d, 1)
    codes = torch.full((N * HP * HP * COUT // 8,), -1, dtype=torch.int32, device="cuda")
    z = torch.empty(N, HP, HP, COUT, dtype=T, device="cuda")
    ops.cl_bn_relu_pool_codes(y, scale, shift, z, codes, N, B, COUT, H, H)
    slabs = ops.cl_layer_bwd_slabs(T, N, CIN, H, H, COUT, K, PAD)
    assert slabs > 0 and (cap is None or slabs == cap)
    dy, dx0, dw0 = _reference(ops, y, gout, x, scale, shift, coef, wk_d, N, B)
    dxa, dwa = _fused(ops, None, None, x, None, None, None, dy, wk_d, N, B, slabs)            # dY given
    dxb, dwb = _fused(ops, y, gout, x, scale, shift, coef, None, wk_d, N, B, slabs)           # recompute
    nan = torch.full_like(scale, float("nan"))     # the code-routed launch reads neither
    dxc, dwc = _fused(ops, y, gout, x, nan, nan, coef, None, wk_d, N, B, slabs, codes=codes)
    same = (dxb == dx0).float().mean().item()
    e = _rel(dwb, dw0)
    with capsys.disabled():
        print(f"\nlayer bwd 28^2 N={N} slabs={slabs}: dW rel {e:.1e}, dX {same:.4f} bit-identical to the separate dgrad")
    # across the apply variants
    assert torch.equal(dxb, dxa) and torch.equal(dwb, dwa)
    assert torch.equal(dxc, dxb) and torch.equal(dwc, dwb)
    # against the three launches
    assert torch.equal(dxb, dx0)
    assert e < 1e-6, e
    if N <= 12:
        w2 = w.flip(2, 3).transpose(0, 1).contiguous().double()
        ref = torch.nn.functional.conv2d(dy.double().permute(0, 3, 1, 2), w2, padding=K - 1 - PAD)
        e64 = _rel(dxb.permute(0, 3, 1, 2), ref)
        w64 = _rel(dwb, _wgrad64(x, dy))
        with capsys.disabled():
            print(f"  against float64: dX rel {e64:.1e}, dW rel {w64:.1e}")
        assert e64 < 5e-3, e64
        assert w64 < 1e-5, w64


DECLINED = [(16, 28, 20, 32), (16, 20, 28, 32), (8, 28, 28, 16), (16, 28, 28, 16), (8, 28, 28, 32),
            (32, 28, 28, 64)]


@pytest.mark.parametrize("Cin,Hh,Ww,Cout", DECLINED, ids=[f"{c}to{o}_{h}x{w_}" for c, h, w_, o in DECLINED])
def test_layer_bwd28_declined_shapes_launch_nothing(Cin, Hh, Ww, Cout):
    from avdino import ops
    from avdino._lib import lib
    N, B, M = 8, 4, 28
    G = N // B
    assert ops.cl_layer_bwd_slabs(T, N, Cin, Hh, Ww, Cout, K, PAD) == 0
    slabs = ops.cl_layer_bwd_slabs(T, N, CIN, H, H, COUT, K, PAD)
    assert slabs > 0
    p, st = ops.p, ops.stream()
    big = N * M * M * 64
    y = torch.zeros(big, device="cuda", dtype=T)
    xin = torch.zeros(big, device="cuda", dtype=T)
    wk_d = torch.zeros(ops.cl_weight_elems(64, 32, K, 1), device="cuda", dtype=T)
    codes = torch.zeros(big // 8, device="cuda", dtype=torch.int32)
    coefs = torch.ones(3, G * 64 * 3, device="cuda")
    dfull, dx = _padded(N * Hh * Ww * Cin, T)
    pfull, parts = _padded(slabs * 64 * 32 * K * K, torch.float32)
    rc = [lib.avd_cl_layer_bwd(p(y), p(y), p(coefs[0]), p(coefs[1]), p(coefs[2]), None, p(xin), p(wk_d),
                               p(dx), p(parts), slabs, 1, N, B, Cin, Hh, Ww, Cout, K, PAD, st),
          lib.avd_cl_layer_bwd(None, None, None, None, None, p(y), p(xin), p(wk_d),
                               p(dx), p(parts), slabs, 1, N, B, Cin, Hh, Ww, Cout, K, PAD, st),
          lib.avd_cl_layer_bwd_codes(p(y), p(y), p(codes), p(coefs[2]), p(xin), p(wk_d), p(dx),
                                     p(parts), slabs, 1, N, B, Cin, Hh, Ww, Cout, K, PAD, st)]
    torch.cuda.synchronize()
    assert rc == [AVD_ERR_SHAPE] * 3, rc
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(parts).all())
    assert _tail_ok(dfull, dx.numel()) and _tail_ok(pfull, parts.numel())


def _engine_step(EN, state, batch, E, D, P):
    from avdino.params import ParamStore
    from avdino.spec import multimodal_dino_sd
    store = ParamStore(multimodal_dino_sd("mse", E, D, P), "cuda")
    store.load_state_dict(state)
    eng = EN.MultiCentralEngine(store, "mse", E, D, P, EN.Hyper(dropout=0.0, fusion_dropout=0.0), act_dtype=T)
    loss = eng.forward(batch).item()
    eng.backward()
    torch.cuda.synchronize()
    grads = {k: store.grad_of(k).detach().clone() for k in store.live_keys}
    return loss, grads, set(eng.ws.bufs)


def test_engine_step_with_fused_28_equals_three_launches():
    from avdino import engine as EN
    from oracle import spec as OS
    from oracle.params import make_multimodal_batch, make_state
    E, D, P, B, G, L = 64, 64, 32, 32, 2, 2
    state = {k: torch.from_numpy(np.array(v)) for k, v in
             make_state(OS.multimodal_dino_spec("mse", E, D, P), 71).items()}
    batch = {k: torch.from_numpy(v).cuda() for k, v in make_multimodal_batch(B, G, L, 72).items()}
    out = {}
    try:
        for on, codes in ((False, True), (True, True), (True, False)):
            EN.ConvBranch.LAYER_BWD_28 = on
            EN.ConvBranch.LAYER_BWD_CODES = codes
            out[on, codes] = _engine_step(EN, state, batch, E, D, P)
    finally:
        EN.ConvBranch.LAYER_BWD_28 = True
        EN.ConvBranch.LAYER_BWD_CODES = True
    (l0, g0, b0), (l1, g1, b1), (l2, g2, b2) = out[False, True], out[True, True], out[True, False]
    # the switch chose the route (both fused layers at once: alternating dX buffers)
    assert "lb_parts2" in b1 and "lb_parts2" not in b0 and "lb_parts1" in b0
    assert {"bwd_dx_lb", "bwd_dx_lb1"} <= b1 and "bwd_dx_lb1" not in b0
    assert any(n.endswith(".pc2") for n in b1) and not any(".pc" in n for n in b2)
    assert l0 == l1 == l2
    pre = "student.audio_encoder.0."
    for k in g0:
        if k == pre + "conv3.weight":
            assert _rel(g1[k], g0[k]) < 1e-6, k
        elif k.startswith((pre + "conv1.", pre + "conv2.", pre + "bn1.", pre + "bn2.")):
            assert _rel(g1[k], g0[k]) < 1e-3, (k, _rel(g1[k], g0[k]))
        else:
            assert torch.equal(g1[k], g0[k]), k
    for k in g1:
        assert torch.equal(g2[k], g1[k]), k
