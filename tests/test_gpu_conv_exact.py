"""Bit-exact integer-data and per-element float64 parity of the conv-block kernels: conv_cl.hip,
conv_ws.hip, conv3.hip, wgrad_cl.hip, wgrad_ws.hip, conv_c1p.hip, bn_cl.hip and the fused backward
launches (lbwd.hip, conv_c1p.hip, c1w3.hip).  test_gpu_cl.py, test_gpu_rect.py and
test_gpu_benchsize.py hold a stored map to one whole-tensor relative L2 norm (5e-3 in bf16),
which a few dozen completely wrong elements pass; this file is where a localised error -- a corner
pixel of the last tile, the last channel octet, a row of a ragged tile, a dropped tap -- fails.

Buffers.  Every read-only operand lies at a 16-byte-aligned offset inside a NaN-filled
allocation whose lead and tail are each a padded halo ((pad W + pad) C elements) + 64 long: a
read outside the tensor that reaches an accumulator poisons the result.  Every output and
partials buffer lies inside an allocation filled with a payload-NaN sentinel that must come back
bit for bit, and is itself pre-filled with NaN: an element not written shows.

a. Integer data (tests/conv_exact_cases.py; the conditions are asserted on the reference by
   tests/test_conv_exact_cases_cpu.py): every product and partial sum is exact in f32 in any
   order, so avd_cl_conv_fwd (with bias), avd_cl_conv_dgrad and avd_cl_conv_wgrad + avd_sum_rows
   must give bf16_rne(float32(exact)) -- torch.equal on the bits, in f32 and bf16; the BatchNorm
   partial rows of the forward (and of avd_cl_conv_fwd_pv about an integer pivot) must sum in
   float64 to the exact sum y, sum y^2 per (channel, group), every row written.  The four
   weights-stationary shapes run with grid_cap {0, 3} x generic_conv {0, 1}: all four the same
   bits, the 14^2 layers that split K over two waves included.  avd_cl_stat_rows is asserted
   against the table's literal: the tiling each case was chosen for.  The (entry point, type)
   pairs the table's rows are declined by return AVD_ERR_SHAPE and write nothing.
b. The BN -> ReLU -> pool block on exact data (scales +-2^k, quarter-integer shifts, power-of-two
   and quarter-integer coefficients, planted ties and dead windows), C in {8, 24, 40}, maps 8x8,
   7x10, 12x20, 5x6, f32 and bf16: avd_cl_bn_relu_pool modes 0 and 2, the code words of
   avd_cl_bn_relu_pool_codes, avd_cl_bn_bwd_apply modes 0 / 1 / 2 (dy rounded to nearest even in
   bf16) bit for bit against the test's own float64 reference; avd_cl_bn_bwd_reduce's rows sum to
   the exact sums.  Mode 1 (global average) is bit-exact where Hp Wp is a power of two and gets
   2 f32 ulps elsewhere (one rounding of the reciprocal, one of the product); its gradient is a
   multiple of Hp Wp, so the backward's division is exact.
c. avd_cl_layer_bwd / avd_cl_layer_bwd_codes (56^2 8 -> 16, 28^2 16 -> 32; grid_cap {0, 3}) and
   avd_cl_bn_bwd_apply_wgrad (16x16 Cout 8 5x5; 8x20 Cout 32 3x3) on the data of b with integer x
   and weights: dx bit for bit, the float64 sum of the slabs exactly, against "dy by the rule of
   csrc/bnapply.h, rounded to bf16, then the exact conv gradients" in float64.
d. Gaussian data on the same table (operands rounded to the storage type on the host): every
   element within the any-order dot-product bound
       |y - y64| <= (Kt + 4) u (sum |x||w| + |bias|),  u = 2^-24,  Kt = Cin K^2
   (input gradient: Kt = Cout K^2; weight gradient: Kt = N Ho Wo + slabs, scale sum |x||dy|),
   a bf16 output adding 2^-8 (|y64| + that bound).  The bound is derived for the f32 route; the
   bf16 MFMA's internal accumulation is undocumented and is held to the same bound.  The largest
   |err| / (u scale) of each test is printed next to Kt + 4 (-s).  Measured on an MI355X:
   MEASURED_MAXIMA below.
"""
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import conv_exact_cases as X  # noqa: E402

# d. the largest |err| / (u scale) seen on an MI355X per (entry point, family of the table):
# (f32, bf16, the smallest bound Kt + 4 among the family's cases).  A bf16 forward / input
# gradient shows 0: whatever the bf16 MFMA's accumulation added stayed inside the store's
# 2^-8 |y64| allowance on every element, so the derived bound holds for it unwidened.
MEASURED_MAXIMA = {
    ("fwd", "generic"): (5.74, 0.0, 76), ("fwd", "cin1"): (4.10, 0.0, 13), ("fwd", "conv3"): (5.14, 0.0, 292),
    ("fwd", "ws"): (None, 0.0, 204),
    ("dgrad", "generic"): (4.72, 0.0, 76), ("dgrad", "conv3"): (4.52, 0.0, 292), ("dgrad", "ws"): (None, 0.0, 404),
    ("wgrad", "generic"): (2.87, 0.95, 106), ("wgrad", "cin1"): (0.65, 0.26, 518),
    ("wgrad", "conv3"): (3.09, 1.27, 36), ("wgrad", "extras"): (1.21, 0.47, 309), ("wgrad", "ws"): (None, 0.54, 408),
}

U = 2.0 ** -24
GUARD = 64
SENT32 = 0x7FC5A5A5            # f32 sentinel bits: a NaN with a payload
SENT16 = 0x7FC5                # bf16 sentinel bits
NAN = float("nan")
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from avdino import ops as _ops
    return _ops


# --------------------------------------------------------------------------------- buffers
class In:
    """A read-only operand at a 16-byte-aligned element offset of a NaN-filled allocation, with at
    least ``halo`` + 64 NaN elements before and after it (integer operands: -1, no valid code)."""

    def __init__(self, vals, halo=0):
        n, al = vals.numel(), 16 // vals.element_size()
        lead = (halo + GUARD + al - 1) // al * al
        self.full = torch.full((lead + n + halo + GUARD,), NAN if vals.dtype.is_floating_point else -1,
                               dtype=vals.dtype, device=DEV)
        self.t = self.full[lead:lead + n].view(vals.shape)
        self.t.copy_(vals)
        assert self.t.data_ptr() % 16 == 0


class Out:
    """An output inside a sentinel-filled allocation (GUARD elements before, GUARD after),
    pre-filled with NaN (integer outputs: -1)."""

    def __init__(self, shape, dtype=torch.float32):
        n = math.prod(shape)
        idt, sent = (torch.int16, SENT16) if dtype == torch.bfloat16 else (torch.int32, SENT32)
        self.raw = torch.full((GUARD + n + GUARD,), sent, dtype=idt, device=DEV)
        self.sent, self.n = sent, n
        self.t = self.raw.view(dtype)[GUARD:GUARD + n].view(shape)
        self.t.fill_(NAN if dtype.is_floating_point else -1)

    def take(self, untouched=False):
        """The result, after checking that nothing around it was written (untouched: nor it)."""
        torch.cuda.synchronize()
        assert bool((self.raw[:GUARD] == self.sent).all()), "a write before the output"
        assert bool((self.raw[GUARD + self.n:] == self.sent).all()), "a write past the output"
        if untouched:
            assert bool(torch.isnan(self.t.float()).all()), "a declined call wrote to its output"
        return self.t.clone()


def same(got, ref, what):
    """torch.equal on the bits, with the count and the first place of a mismatch."""
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    idt = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    bad = got.contiguous().view(idt) != ref.contiguous().view(idt)
    if bool(bad.any()):
        at = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: "
                             f"got {got[at].item()!r}, exact {ref[at].item()!r}")


def nhwc(t64, T):
    """NCHW float64 (host) -> NHWC of type T on the device."""
    return t64.permute(0, 2, 3, 1).contiguous().to(T).to(DEV)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def stored(t64, T):
    """The float64 reference as the kernel stores it: f32 (exact), then bf16 by RNE."""
    return t64.float().to(T)


def vec(t64):
    return In(t64.reshape(-1).float().to(DEV))


def layout(ops, w64, dgrad, T):
    """The MFMA weight layout of w, placed between NaNs."""
    Co, Ci, K, _ = w64.shape
    wk = torch.empty(ops.cl_weight_elems(Co, Ci, K, dgrad), device=DEV, dtype=T)
    ops.cl_weight_layout(w64.float().to(DEV), wk, dgrad)
    return In(wk)


# ------------------------------------------------------------------------- the three calls
def run_fwd(ops, case, x, w, b, T, pivot=None, stats=True):
    """avd_cl_conv_fwd[_pv] -> (y NCHW, stats [Cout, G, R, 2] or None, R)."""
    N, B, Cin, H, W, Cout, K, pad = case[:8]
    Ho, Wo = X.out_hw(case)
    xb, wk, bb = In(nhwc(x, T), (pad * W + pad) * Cin), layout(ops, w, 0, T), vec(b)
    y = Out((N, Ho, Wo, Cout), T)
    R = ops.cl_stat_rows(Ho, Wo, B, K, Cin, Cout, T) if stats else 0
    st = Out((Cout, N // B, R, 2)) if stats else None
    pv = vec(pivot) if pivot is not None else None
    ops.cl_conv_fwd(xb.t, wk.t, bb.t, y.t, st.t if stats else None, N, B, Cin, H, W, Cout, K, pad,
                    pivot=pv.t if pv else None)
    return nchw(y.take()), st.take() if stats else None, R


def run_dgrad(ops, case, dy, w, T):
    N, B, Cin, H, W, Cout, K, pad = case[:8]
    Ho, Wo = X.out_hw(case)
    dp = K - 1 - pad
    dyb, wk = In(nhwc(dy, T), (dp * Wo + dp) * Cout), layout(ops, w, 1, T)
    dx = Out((N, H, W, Cin), T)
    ops.cl_conv_dgrad(dyb.t, wk.t, dx.t, N, Cin, H, W, Cout, K, pad)
    return nchw(dx.take())


def run_wgrad(ops, case, x, dy, T):
    """avd_cl_conv_wgrad + avd_sum_rows -> (dw [Cout, Cin, K, K] f32, slabs [chunks, ...] f32)."""
    N, B, Cin, H, W, Cout, K, pad = case[:8]
    Ho, Wo = X.out_hw(case)
    xb, dyb = In(nhwc(x, T), (pad * W + pad) * Cin), In(nhwc(dy, T), (pad * Wo + pad) * Cout)
    chunks = ops.cl_wgrad_chunks(N, Cout, Cin, K)
    assert chunks > 0
    cols = Cout * Cin * K * K
    parts, dw = Out((chunks, cols)), Out((Cout, Cin, K, K))
    ops.cl_conv_wgrad(xb.t, dyb.t, parts.t, N, Cin, H, W, Cout, K, pad)
    ops.sum_rows(parts.t, chunks, cols, dw.t)
    return dw.take(), parts.take().view(chunks, Cout, Cin, K, K)


def want_rows(case, dt):
    r = case[9][dt == "bf16"]
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count if r == "4cu" else r


def check_stats(st, ref, what):
    assert not bool(torch.isnan(st).any()), f"{what}: a partial row was not written"
    got = st.double().sum(2).cpu()
    bad = got != ref
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} (channel, group, moment) sums "
                                 f"differ, first at {tuple(bad.nonzero()[0].tolist())}: "
                                 f"{got[bad][0].item()} != {ref[bad][0].item()}")


FWD, _ = X.run_list("f")
DGRAD, _ = X.run_list("d")
WGRAD, _ = X.run_list("w")


def pid(p):
    return f"{X.cid(p[0])}-{p[1]}"


# ============================================================ a. integer data, bit for bit
@pytest.mark.parametrize("case,dt", FWD, ids=[pid(p) for p in FWD])
def test_conv_fwd_exact(ops, case, dt):
    T, B = DT[dt], case[1]
    x, w, b = X.fwd_data(case, "map")
    y, st, R = run_fwd(ops, case, x, w, b, T)
    assert R == want_rows(case, dt), f"avd_cl_stat_rows {R}: not the tiling this case was chosen for"
    same(y, stored(X.fwd_ref(case, "map")[0], T), "y")
    assert not bool(torch.isnan(st).any()), "a partial row was not written"
    # {-1, 0, 1} data: the stored y is the exact y, and so are the sums
    x, w, b = X.fwd_data(case, "stats")
    ys = X.fwd_ref(case, "stats")[0]
    y, st, _ = run_fwd(ops, case, x, w, b, T)
    same(y, stored(ys, T), "y (stats data)")
    check_stats(st, X.stats_ref(ys, B), "sum y, sum y^2")


@pytest.mark.parametrize("case,dt", DGRAD, ids=[pid(p) for p in DGRAD])
def test_conv_dgrad_exact(ops, case, dt):
    T = DT[dt]
    dx = run_dgrad(ops, case, X.bwd_data(case, "map"), X.fwd_data(case, "map")[1], T)
    same(dx, stored(X.dgrad_ref(case, "map")[0], T), "dx")


@pytest.mark.parametrize("case,dt", WGRAD, ids=[pid(p) for p in WGRAD])
def test_conv_wgrad_exact(ops, case, dt):
    T = DT[dt]
    dw, parts = run_wgrad(ops, case, X.fwd_data(case, "map")[0], X.bwd_data(case, "map"), T)
    ref = X.wgrad_ref(case, "map")[0]
    assert not bool(torch.isnan(parts).any()), "a slab element was not written"
    assert torch.equal(parts.double().sum(0).cpu(), ref), "the float64 sum of the slabs is not the exact dW"
    same(dw, ref.float(), "dw")


DECLINED = X.declined_list()


@pytest.mark.parametrize("kind,case,dt", DECLINED, ids=[f"{k}-{X.cid(c)}-{d}" for k, c, d in DECLINED])
def test_declined_channel_counts(ops, kind, case, dt):
    """The generic forward / input gradient exist for 8, 16, 32, 64 (3x3: 128, 256) channels of the
    map they read (include/avdino.h): another count is AVD_ERR_SHAPE before any launch."""
    from avdino._lib import AvdError
    T = DT[dt]
    N, B, Cin, H, W, Cout, K, pad = case[:8]
    Ho, Wo = X.out_hw(case)
    x, w, _ = X.fwd_data(case, "stats")
    wk = layout(ops, w, kind == "d", T)
    if kind == "f":
        src, out = In(nhwc(x, T)), Out((N, Ho, Wo, Cout), T)
        with pytest.raises(AvdError, match="AVD_ERR_SHAPE"):
            ops.cl_conv_fwd(src.t, wk.t, None, out.t, None, N, B, Cin, H, W, Cout, K, pad)
    else:
        src, out = In(nhwc(X.bwd_data(case, "map"), T)), Out((N, H, W, Cin), T)
        with pytest.raises(AvdError, match="AVD_ERR_SHAPE"):
            ops.cl_conv_dgrad(src.t, wk.t, out.t, N, Cin, H, W, Cout, K, pad)
    out.take(untouched=True)


@pytest.mark.parametrize("case", X.CONV3, ids=X.cid)
def test_c3_conv_eval_exact(ops, case):
    """avd_c3_conv_eval (conv3.hip's eval-mode layer: conv -> fixed affine -> ReLU -> 2x2 max-pool
    in one launch), mode 0, on the integer data with scale = +-2^k and quarter-integer shifts:
    bf16_rne of the affine of the bf16_rne conv output, pooled -- bit for bit.  The rows 31..46
    wide are served like every other width up to 62."""
    T = torch.bfloat16
    N, B, Cin, H, W, Cout, K, pad = case[:8]
    x, w, b = X.fwd_data(case, "map")
    if not ops.c3_eval_serves(N, H, W, Cin, Cout, 0):
        # (a map whose pooling tile does not fit: the call launches nothing and says so)
        assert not 31 <= W <= 46, "avd_c3_eval_serves declines a 31..46 wide map"
        xb, wk, out = In(nhwc(x, T)), layout(ops, w, 0, T), Out((N, H // 2, W // 2, Cout), T)
        one = vec(torch.ones(Cout, dtype=F64))
        assert not ops.c3_conv_eval(xb.t, wk.t, None, one.t, one.t, out.t, 0, N, H, W, Cin, Cout)
        out.take(untouched=True)
        return
    g = torch.Generator().manual_seed(17 + Cout + W)
    scale = torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0).double() * 2.0 ** torch.randint(-3, 1, (Cout,), generator=g)
    shift = torch.randint(-8, 9, (Cout,), generator=g).double() / 4
    y = stored(X.fwd_ref(case, "map")[0], T).double()
    z = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    assert torch.equal(z.float().double(), z)               # the kernel's one fmaf is exact
    pooled, _ = X.pool_ref(torch.where(z > 0, z, torch.zeros_like(z)))
    xb, wk, bb = In(nhwc(x, T), (W + 1) * Cin), layout(ops, w, 0, T), vec(b)
    out = Out((N, H // 2, W // 2, Cout), T)
    assert ops.c3_conv_eval(xb.t, wk.t, bb.t, vec(scale).t, vec(shift).t, out.t, 0, N, H, W, Cin, Cout)
    same(nchw(out.take()), stored(pooled, T), "pooled map")


# ---- the weights-stationary mid layers: grid_cap {0, 3} x generic_conv {0, 1}, bf16
WS_RUNS = [(c, cap, gen) for c in X.WS for cap in (0, 3) for gen in (0, 1)]
WS_IDS = [f"{X.cid(c)}-cap{cap}-{'generic' if gen else 'ws'}" for c, cap, gen in WS_RUNS]


@pytest.mark.parametrize("case,cap,generic", WS_RUNS, ids=WS_IDS)
def test_ws_conv_fwd_exact(ops, case, cap, generic, avd_opts):
    avd_opts(grid_cap=cap, generic_conv=generic)
    T, B = torch.bfloat16, case[1]
    Ho, Wo = X.out_hw(case)
    x, w, b = X.fwd_data(case, "map")
    y, st, R = run_fwd(ops, case, x, w, b, T)
    same(y, stored(X.fwd_ref(case, "map")[0], T), "y")
    assert not bool(torch.isnan(st).any()), "a partial row was not written"
    pivots = bool(ops.cl_stat_pivot(Ho, Wo, B, case[6], case[2], case[5], T))
    assert pivots == (not generic)
    if generic:
        assert R == case[9][1]                       # plan_cl's tiling of this shape
    elif cap:
        assert R % cap == 0                          # the persistent grid: cap blocks
    x, w, b = X.fwd_data(case, "stats")
    ys = X.fwd_ref(case, "stats")[0]
    y, st, _ = run_fwd(ops, case, x, w, b, T)
    same(y, stored(ys, T), "y (stats data)")
    check_stats(st, X.stats_ref(ys, B), "sum y, sum y^2")
    if pivots:
        pv = X.pivot_of(case)
        y, st, _ = run_fwd(ops, case, x, w, b, T, pivot=pv)
        same(y, stored(ys, T), "y (pivot call)")
        check_stats(st, X.stats_ref(ys, B, pv), "sum (y - K), sum (y - K)^2")


@pytest.mark.parametrize("case,cap,generic", WS_RUNS, ids=WS_IDS)
def test_ws_conv_dgrad_exact(ops, case, cap, generic, avd_opts):
    avd_opts(grid_cap=cap, generic_conv=generic)
    T = torch.bfloat16
    dx = run_dgrad(ops, case, X.bwd_data(case, "map"), X.fwd_data(case, "map")[1], T)
    same(dx, stored(X.dgrad_ref(case, "map")[0], T), "dx")


@pytest.mark.parametrize("case,cap,generic", WS_RUNS, ids=WS_IDS)
def test_ws_conv_wgrad_exact(ops, case, cap, generic, avd_opts):
    avd_opts(grid_cap=cap, generic_conv=generic)
    dw, parts = run_wgrad(ops, case, X.fwd_data(case, "map")[0], X.bwd_data(case, "map"), torch.bfloat16)
    ref = X.wgrad_ref(case, "map")[0]
    if cap and not generic and case[7] == 2:
        assert parts.shape[0] == cap                 # 3 slabs over 4 samples
    assert not bool(torch.isnan(parts).any()), "a slab element was not written"
    assert torch.equal(parts.double().sum(0).cpu(), ref), "the float64 sum of the slabs is not the exact dW"
    same(dw, ref.float(), "dw")


# ======================================================== b. BN -> ReLU -> pool block, exact
POOL = [(C, H, W, dt) for C in X.POOL_C for H, W in X.POOL_HW for dt in ("f32", "bf16")]
POOL_IDS = [f"C{C}-{H}x{W}-{dt}" for C, H, W, dt in POOL]


class Block:
    """The block's operands on the device (NHWC, between NaNs) and its float64 reference."""

    def __init__(self, C, H, W, T):
        self.N, self.B, self.C, self.H, self.W, self.T = X.POOL_N, X.POOL_B, C, H, W, T
        self.Hp, self.Wp = H // 2, W // 2
        self.d = X.block_data(C, H, W)
        y, scale, shift, coef, mean, invstd, gout = self.d
        self.y = In(nhwc(y, T), W * C)
        self.scale, self.shift, self.coef = vec(scale), vec(shift), vec(coef)
        self.mean, self.invstd = vec(mean), vec(invstd)

    def gout(self, mode):
        """(device gradient in the mode's layout, the gradient of the pooled map in float64)"""
        g = self.d[6]
        if mode == 0:
            return In(nhwc(g, self.T)), g
        if mode == 2:
            return In(g.reshape(self.N, -1).float().to(DEV)), g
        g1 = g[:, :, 0, 0] * (self.Hp * self.Wp)          # a multiple of Hp Wp: exact division
        return In(g1.float().to(DEV)), (g1 / (self.Hp * self.Wp)).view(self.N, self.C, 1, 1).expand_as(g)

    def ref(self, mode, round_dy):
        y, scale, shift, coef, mean, invstd, _ = self.d
        return X.block_ref(y, scale, shift, coef, mean, invstd, self.gout(mode)[1].contiguous(), self.B, round_dy)


@pytest.mark.parametrize("C,H,W,dt", POOL, ids=POOL_IDS)
def test_bn_relu_pool_exact(ops, C, H, W, dt):
    T = DT[dt]
    k = Block(C, H, W, T)
    N, B, Hp, Wp = k.N, k.B, k.Hp, k.Wp
    pooled, nib = k.ref(0, False)[:2]
    out = Out((N, Hp, Wp, C), T)
    ops.cl_bn_relu_pool(k.y.t, k.scale.t, k.shift.t, out.t, 0, N, B, C, H, W)
    same(nchw(out.take()), stored(pooled, T), "mode 0")
    out = Out((N, C * Hp * Wp))
    ops.cl_bn_relu_pool(k.y.t, k.scale.t, k.shift.t, out.t, 2, N, B, C, H, W)
    same(out.take(), pooled.reshape(N, -1).float(), "mode 2")
    out = Out((N, C))
    ops.cl_bn_relu_pool(k.y.t, k.scale.t, k.shift.t, out.t, 1, N, B, C, H, W)
    got, mean = out.take().cpu(), pooled.mean((2, 3))
    if (Hp * Wp) & (Hp * Wp - 1) == 0:
        same(got, mean.float(), "mode 1")
    else:       # 2 f32 ulps of the exact mean: the reciprocal's rounding and the product's
        ulp = torch.ldexp(torch.ones_like(mean), torch.frexp(mean)[1] - 24)
        assert bool(((got.double() - mean).abs() <= 2 * ulp).all()), "mode 1"
    if dt == "bf16":
        out, codes = Out((N, Hp, Wp, C), T), Out((N, Hp, Wp, C // 8), torch.int32)
        ops.cl_bn_relu_pool_codes(k.y.t, k.scale.t, k.shift.t, out.t, codes.t.view(-1), N, B, C, H, W)
        same(nchw(out.take()), stored(pooled, T), "codes call: out")
        words = (nib.permute(0, 2, 3, 1).reshape(N, Hp, Wp, C // 8, 8) << (4 * torch.arange(8))).sum(-1)
        got = codes.take().cpu().to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(got, words), "code words"


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C,H,W,dt", POOL, ids=POOL_IDS)
def test_bn_bwd_exact(ops, C, H, W, dt, mode):
    T = DT[dt]
    k = Block(C, H, W, T)
    N, B = k.N, k.B
    g, _ = k.gout(mode)
    _p, _n, _dz, dy, sums, _a = k.ref(mode, dt == "bf16")
    out = Out((N, H, W, C), T)
    ops.cl_bn_bwd_apply(k.y.t, g.t, mode, k.scale.t, k.shift.t, k.coef.t, out.t, N, B, C, H, W)
    same(nchw(out.take()), stored(dy, T), "dy")
    R = ops.cl_bn_bwd_rows(B, C, H, W, T)
    parts = Out((C, N // B, R, 2))
    ops.cl_bn_bwd_reduce(k.y.t, g.t, mode, k.scale.t, k.shift.t, k.mean.t, k.invstd.t, parts.t, N, B, C, H, W)
    check_stats(parts.take(), sums, "sum dz, sum dz xhat")


# ======================================================== c. fused backward launches, exact
def fused_operands(ops, case, T=torch.bfloat16):
    N, B, Cin, H, W, Cout, K, pad = case
    r = X.fused_ref(case)
    dev = dict(y=In(nhwc(r["y"], T), W * Cout), gout=In(nhwc(r["gout"], T)), x=In(nhwc(r["x"], T), (pad * W + pad) * Cin),
               scale=vec(r["scale"]), shift=vec(r["shift"]), coef=vec(r["coef"]))
    return r, dev


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("case", X.LAYER_BWD, ids=X.cid)
def test_layer_bwd_exact(ops, case, cap, avd_opts):
    """avd_cl_layer_bwd (recomputed routing) and avd_cl_layer_bwd_codes (the forward's words; scale
    and shift NaN: not read): dx and the summed slabs against the float64 reference."""
    avd_opts(grid_cap=cap)
    T = torch.bfloat16
    N, B, Cin, H, W, Cout, K, pad = case
    r, d = fused_operands(ops, case)
    wk_d = layout(ops, r["w"], 1, T)
    slabs = ops.cl_layer_bwd_slabs(T, N, Cin, H, W, Cout, K, pad)
    assert slabs > 0 and (not cap or slabs == cap)
    pooled, codes = Out((N, H // 2, W // 2, Cout), T), Out((N * (H // 2) * (W // 2) * Cout // 8,), torch.int32)
    ops.cl_bn_relu_pool_codes(d["y"].t, d["scale"].t, d["shift"].t, pooled.t, codes.t, N, B, Cout, H, W)
    words = In(codes.take())
    nan = vec(torch.full_like(r["scale"], NAN))
    cols = Cout * Cin * K * K
    for what, cw, sc, sf in (("recomputed routing", None, d["scale"], d["shift"]), ("code-routed", words, nan, nan)):
        dx, parts = Out((N, H, W, Cin), T), Out((slabs, cols))
        ops.cl_layer_bwd(d["y"].t, d["gout"].t, sc.t, sf.t, d["coef"].t, None, d["x"].t, wk_d.t, dx.t,
                         parts.t, slabs, N, B, Cin, H, W, Cout, K, pad, codes=cw.t if cw else None)
        same(nchw(dx.take()), stored(r["dx"], T), f"{what}: dx")
        p = parts.take()
        assert not bool(torch.isnan(p).any()), f"{what}: a slab element was not written"
        assert torch.equal(p.double().sum(0).cpu().view(Cout, Cin, K, K), r["dw"]), f"{what}: the slabs' sum is not dW"
        dw = Out((Cout, Cin, K, K))
        ops.sum_rows(p, slabs, cols, dw.t)
        same(dw.take(), r["dw"].float(), f"{what}: dw")


@pytest.mark.parametrize("case", X.APPLY_WGRAD, ids=X.cid)
def test_apply_wgrad_exact(ops, case):
    T = torch.bfloat16
    N, B, Cin, H, W, Cout, K, pad = case
    r, d = fused_operands(ops, case)
    slabs = ops.cl_apply_wgrad_slabs(T, N, Cin, H, W, Cout, K, pad)
    assert slabs > 0
    cols = Cout * K * K
    parts = Out((slabs, cols))
    ops.cl_bn_bwd_apply_wgrad(d["y"].t, d["gout"].t, d["scale"].t, d["shift"].t, d["coef"].t, d["x"].t, parts.t,
                              N, B, Cin, H, W, Cout, K, pad)
    p = parts.take()
    assert not bool(torch.isnan(p).any()), "a slab element was not written"
    assert torch.equal(p.double().sum(0).cpu().view(Cout, Cin, K, K), r["dw"]), "the slabs' sum is not dW"


# ========================================================= d. Gaussian data, per-element band
class Report:
    """The largest error ratio of a test and the bound it was held to, printed once."""

    def __init__(self, capsys, what):
        self.capsys, self.what = capsys, what

    def check(self, got, ref, scale, kt, T):
        """|got - ref| <= (kt + 4) u scale, a bf16 output adding 2^-8 (|ref| + that bound)."""
        bound = (kt + 4) * U * scale
        err = (got.double().cpu() - ref).abs()
        assert not bool(torch.isnan(err).any()), "NaN in the result (an element not written, or a padded read)"
        if T == torch.bfloat16:
            err = (err - 2.0 ** -8 * (ref.abs() + bound)).clamp_min(0)
        assert bool((err[scale == 0] == 0).all()), "an error where the bound is zero"
        r = float((err / (U * scale.clamp_min(1e-300))).max())
        with self.capsys.disabled():
            print(f"\n[conv-exact] {self.what}: max |err|/(u scale) {r:.2f}, bound {kt + 4}", end="")
        assert r <= kt + 4, f"{self.what}: |err| / (u scale) = {r:.2f} > {kt + 4}"


BAND_F, _ = X.run_list("f", X.ALL)
BAND_D, _ = X.run_list("d", X.ALL)
BAND_W, _ = X.run_list("w", X.ALL)
BAND_F, BAND_D, BAND_W = ([(c, dt) for c, dt in rows if c not in X.WS or dt == "bf16"] for rows in (BAND_F, BAND_D, BAND_W))


@pytest.mark.parametrize("case,dt", BAND_F, ids=[pid(p) for p in BAND_F])
def test_conv_fwd_band(ops, case, dt, capsys):
    T = DT[dt]
    x, w, b = X.fwd_data(case, "gauss")
    y64, scale = X.fwd_ref(case, "gauss", dt)
    y, _, _ = run_fwd(ops, case, X.rounded(x, dt), X.rounded(w, dt), b, T, stats=False)
    Report(capsys, f"fwd {pid((case, dt))}").check(y, y64, scale, case[2] * case[6] ** 2, T)


@pytest.mark.parametrize("case,dt", BAND_D, ids=[pid(p) for p in BAND_D])
def test_conv_dgrad_band(ops, case, dt, capsys):
    T = DT[dt]
    dx64, scale = X.dgrad_ref(case, "gauss", dt)
    dx = run_dgrad(ops, case, X.rounded(X.bwd_data(case, "gauss"), dt), X.rounded(X.fwd_data(case, "gauss")[1], dt), T)
    Report(capsys, f"dgrad {pid((case, dt))}").check(dx, dx64, scale, case[5] * case[6] ** 2, T)


@pytest.mark.parametrize("case,dt", BAND_W, ids=[pid(p) for p in BAND_W])
def test_conv_wgrad_band(ops, case, dt, capsys):
    T = DT[dt]
    dw64, scale = X.wgrad_ref(case, "gauss", dt)
    dw, parts = run_wgrad(ops, case, X.rounded(X.fwd_data(case, "gauss")[0], dt), X.rounded(X.bwd_data(case, "gauss"), dt), T)
    Ho, Wo = X.out_hw(case)
    Report(capsys, f"wgrad {pid((case, dt))}").check(dw, dw64, scale, case[0] * Ho * Wo + parts.shape[0], torch.float32)
