"""The forward pool's routing codes (avd_cl_bn_relu_pool_codes, csrc/bn_cl.hip) and the fused
audio-conv2 layer backward routed by them (avd_cl_layer_bwd_codes, csrc/lbwd.hip AP = 2):

* the pooling call with codes writes the pooled map of ops.cl_bn_relu_pool bit for bit; a code
  nibble is 0 exactly where the pooled value is 0, never above 4, and at every coded position
  relu(bn(y)) recomputed in float64 from the bf16 y rounds (f64 -> f32 as the kernel's one fmaf
  does, -> bf16 as its store does) to the pooled value;
* the code-routed fused backward gives the dX and the summed dW of the recompute variant (the
  cl_layer_bwd(y, gout, ...) call) bit for bit at the same slab count, and stays inside
  test_gpu_lbwd.py's bands against apply + dgrad + wgrad;
* an engine step with ConvBranch.LAYER_BWD_CODES on equals the step with it off: loss and every
  gradient tensor bit for bit.

The layer is fixed (56x56, 8 -> 16, 5x5); N, B and the grid cap choose: blocks that start
mid-sample with continuation tiles and BN-group changes inside a block's range (12, 4, cap 5),
one tile per block (10, 5), APPLY_GMAX = 8 groups (8, 1, cap 3), a single sample (1, 1, cap 2).
The operands are test_gpu_lbwd.py's with negative scales, exact in-window ties (first max
decides), windows whose BN output is <= 0 everywhere (code 0) and zero pooled gradients."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = torch.bfloat16
F64 = torch.float64
CIN, COUT, K, PAD, H = 8, 16, 5, 2, 56
HP = H // 2

CASES = [(12, 4, 5), (10, 5, None), (8, 1, 3), (1, 1, 2)]
IDS = ["capped", "one_tile_per_block", "gmax_groups", "single_sample"]


@functools.lru_cache(maxsize=None)
def _operands(N, B):
    g = torch.Generator(device="cuda").manual_seed(160 + N)
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


def _pool(ops, y, scale, shift, N, B, codes=None, plain=False):
    out = torch.full((N, HP, HP, COUT), float("nan"), device="cuda").to(T)
    if plain:
        ops.cl_bn_relu_pool(y, scale, shift, out, 0, N, B, COUT, H, H)
    else:
        ops.cl_bn_relu_pool_codes(y, scale, shift, out, codes, N, B, COUT, H, H)
    return out


def _codes(ops, y, scale, shift, N, B):
    codes = torch.full((N * HP * HP * COUT // 8,), -1, dtype=torch.int32, device="cuda")
    return _pool(ops, y, scale, shift, N, B, codes), codes


def _nibbles(codes, N):
    """[N, HP, HP, COUT] int64: the nibble of every (pooled pixel, channel)."""
    c = codes.view(N, HP, HP, COUT // 8, 1).to(torch.int64) & 0xFFFFFFFF
    return ((c >> (4 * torch.arange(8, device="cuda"))) & 15).reshape(N, HP, HP, COUT)


def _reference(ops, y, gout, x, scale, shift, coef, wk_d, N, B):
    dy = torch.empty_like(y)
    ops.cl_bn_bwd_apply(y, gout, 0, scale, shift, coef, dy, N, B, COUT, H, H)
    dx = torch.empty(N, H, H, CIN, dtype=T, device="cuda")
    ops.cl_conv_dgrad(dy, wk_d, dx, N, CIN, H, H, COUT, K, PAD)
    nch = ops.cl_wgrad_chunks(N, COUT, CIN, K)
    parts = torch.empty(nch * COUT * CIN * K * K, device="cuda")
    ops.cl_conv_wgrad(x, dy, parts, N, CIN, H, H, COUT, K, PAD)
    dw = torch.empty(COUT * CIN * K * K, device="cuda")
    ops.sum_rows(parts, nch, COUT * CIN * K * K, dw)
    return dy, dx, dw


def _fused(ops, y, gout, x, scale, shift, coef, wk_d, N, B, slabs, codes):
    parts = torch.full((slabs * COUT * CIN * K * K,), float("nan"), device="cuda")
    dx = torch.full((N, H, H, CIN), float("nan"), device="cuda").to(T)
    ops.cl_layer_bwd(y, gout, scale, shift, coef, None, x, wk_d, dx, parts, slabs, N, B, CIN, H, H, COUT, K,
                     PAD, codes=codes)
    dw = torch.empty(COUT * CIN * K * K, device="cuda")
    ops.sum_rows(parts, slabs, COUT * CIN * K * K, dw)
    return dx, dw


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("N,B,cap", CASES, ids=IDS)
def test_pool_codes(N, B, cap, avd_opts):
    from avdino import ops
    if cap:
        avd_opts(grid_cap=cap)
    y, _gout, _x, scale, shift, _coef, _w = _operands(N, B)
    z0 = _pool(ops, y, scale, shift, N, B, plain=True)
    z1, codes = _codes(ops, y, scale, shift, N, B)
    z2 = _pool(ops, y, scale, shift, N, B, codes=None)  # a null codes pointer: no stores, same map
    torch.cuda.synchronize()
    assert torch.equal(z1, z0) and torch.equal(z2, z0)
    nib = _nibbles(codes, N)
    assert int(nib.max()) <= 4
    assert torch.equal(nib == 0, z0 == 0)
    # the operands exercise the routing: dead windows, all four argmax positions
    assert all(bool((nib == v).any()) for v in range(5))
    G = N // B
    sc = scale.double().view(G, 1, 1, 1, COUT).expand(G, B, H, H, COUT).reshape(N, H, H, COUT)
    sf = shift.double().view(G, 1, 1, 1, COUT).expand(G, B, H, H, COUT).reshape(N, H, H, COUT)
    a = torch.relu(y.double() * sc + sf).to(torch.float32)     # f64 -> f32: the kernel's one fmaf
    win = torch.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]], -1)
    coded = nib > 0
    at = torch.gather(win, -1, (nib - 1).clamp_min(0).unsqueeze(-1))
    assert torch.equal(at.squeeze(-1).to(T)[coded], z0[coded])  # -> bf16: its store
    # the coded pixel is the window's first max (compared in f32, before the store's rounding)
    k = torch.arange(4, device="cuda")
    bad = ((win > at) | ((k < (nib - 1).unsqueeze(-1)) & (win >= at))) & coded.unsqueeze(-1)
    assert not bool(bad.any())


@pytest.mark.parametrize("N,B,cap", CASES, ids=IDS)
def test_code_routed_layer_bwd_equals_recompute(N, B, cap, avd_opts, capsys):
    from avdino import ops
    if cap:
        avd_opts(grid_cap=cap)
    y, gout, x, scale, shift, coef, w = _operands(N, B)
    wk_d = torch.empty(ops.cl_weight_elems(COUT, CIN, K, 1), dtype=T, device="cuda")
    ops.cl_weight_layout(w, wk_d, 1)
    _z, codes = _codes(ops, y, scale, shift, N, B)
    slabs = ops.cl_layer_bwd_slabs(T, N, CIN, H, H, COUT, K, PAD)
    assert slabs > 0 and (cap is None or slabs == cap)
    dx1, dw1 = _fused(ops, y, gout, x, scale, shift, coef, wk_d, N, B, slabs, None)       # recompute
    # the code-routed launch reads neither scale nor shift: NaN there must not reach its output
    nan = torch.full_like(scale, float("nan"))
    dx2, dw2 = _fused(ops, y, gout, x, nan, nan, coef, wk_d, N, B, slabs, codes)
    dy, dx0, dw0 = _reference(ops, y, gout, x, scale, shift, coef, wk_d, N, B)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx1)
    assert torch.equal(dw2, dw1)
    d, r = (dx2.float() - dx0.float()).abs(), dx0.float().abs()
    same = (dx2 == dx0).float().mean().item()
    e = _rel(dw2, dw0)
    with capsys.disabled():
        print(f"\ncode-routed layer bwd N={N}: dW rel {e:.1e}, dX {same:.4f} bit-identical to the separate dgrad")
    assert bool((d <= r * 2.0 ** -7 + 1e-5 * r.max()).all()) and same >= 0.97
    assert e < 1e-6, e


def test_engine_step_with_codes_equals_recompute():
    from avdino import engine as EN
    from avdino.params import ParamStore
    from avdino.spec import multimodal_dino_sd
    from oracle import spec as OS
    from oracle.params import make_multimodal_batch, make_state
    E, D, P, B, G, L = 64, 64, 32, 32, 2, 2
    state = {k: torch.from_numpy(np.array(v)) for k, v in
             make_state(OS.multimodal_dino_spec("mse", E, D, P), 71).items()}
    batch = {k: torch.from_numpy(v).cuda() for k, v in make_multimodal_batch(B, G, L, 72).items()}
    out, used = {}, {}
    for on in (False, True):
        EN.ConvBranch.LAYER_BWD_CODES = on
        try:
            store = ParamStore(multimodal_dino_sd("mse", E, D, P), "cuda")
            store.load_state_dict(state)
            eng = EN.MultiCentralEngine(store, "mse", E, D, P, EN.Hyper(dropout=0.0, fusion_dropout=0.0),
                                        act_dtype=T)
            loss = eng.forward(batch).item()
            eng.backward()
            torch.cuda.synchronize()
            out[on] = (loss, {k: store.grad_of(k).detach().clone() for k in store.live_keys})
            used[on] = any(".pc" in name for name in eng.ws.bufs)
        finally:
            EN.ConvBranch.LAYER_BWD_CODES = True
    assert used[True] and not used[False]          # the switch chose the route
    (l0, g0), (l1, g1) = out[False], out[True]
    assert l0 == l1
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
