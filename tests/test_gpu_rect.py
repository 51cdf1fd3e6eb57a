"""The conv-block entry points of include/avdino.h on rectangular maps (H != W).

Every entry point below takes H and W separately, and the engine only ever passes squares.  The
contract pinned here: for H != W an entry point either computes the right answer or declines (its
sizing query returns 0 / it returns AVD_ERR_SHAPE before any launch) -- it is never wrong with
AVD_OK.  TABLE is that contract as a literal: entry point, shape, served or declined.  Every
"served" row is run in both orientations and compared with the float64 oracle (and, where the
square test of the same entry point asserts it, bit for bit with the unfused launches) under the
tolerances of that square test:
  tests/test_gpu_cl.py: stored maps rel-L2 2e-6 (f32) / 5e-3 (bf16), f32 reductions 1e-5;
  torch.equal wherever a fused route is defined as bit-identical to the launches it replaces.
(Those norms cannot see a few wrong elements: localised errors are caught bit for bit by
tests/test_gpu_conv_exact.py, rectangular maps included.)
A zero row count or AVD_ERR_SHAPE on a "served" row fails; a "declined" row must answer 0 from its
sizing query, and where the host check stands before the first launch the entry point itself is
called and must return AVD_ERR_SHAPE with its sentinel-filled outputs untouched.

So that a transposed index shows at once, x[n, h, w, c] carries a term that grows with h and a
different one that falls with w, and BN group g is scaled by 10^g (the rel-L2 bands are then
applied per group).  So that a transposed stride cannot leave the test's own memory, every device
buffer is allocated as if the map were max(H, W) square, plus a tail, NaN-filled (-1 for integer
codes); the kernels see the leading N*H*W*C elements and the rest must come back untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = pytest.importorskip("torch.nn.functional")

from oracle import numpy_oracle as O  # noqa: E402
from tests.test_gpu_cl import DT, TOL, bf, host, nchw, nhwc, rel  # noqa: E402

BF = torch.bfloat16
F64 = torch.float64
S, D = "served", "declined"
AVD_ERR_SHAPE, AVD_ERR_ARG = -1, -4
TAIL = 512

CASES = {  # name: Cin, Cout, K, pad, N, B
    "R1": (8, 16, 5, 2, 4, 2),      # conv_cl generic, ragged tiles on both axes
    "R2": (1, 32, 3, 1, 4, 2),      # conv_c1 generic (f32); c1w3 first-layer routes (bf16)
    "R3": (1, 8, 5, 2, 4, 2),       # bf16: the pixel-pair route (conv_c1p.hip); f32: generic
    "R4": (32, 64, 3, 1, 3, 3),     # bf16: conv3.hip; f32: generic
    "R5": (32, 64, 5, 0, 3, 3),     # unpadded output extents (14x10 -> 10x6)
}


def both(entry, case, H, W, verdict=S):
    return [(entry, case, H, W, verdict), (entry, case, W, H, verdict)]


TABLE = [  # entry point(s), case, H, W, served / declined
    *both("avd_cl_conv_fwd", "R1", 12, 20), *both("avd_cl_conv_fwd", "R2", 8, 20),
    *both("avd_cl_conv_fwd", "R3", 16, 48), *both("avd_cl_conv_fwd", "R3", 16, 112),
    *both("avd_cl_conv_fwd", "R4", 10, 24), *both("avd_cl_conv_fwd", "R5", 14, 10),
    *both("avd_cl_conv_dgrad", "R1", 12, 20), *both("avd_cl_conv_dgrad", "R4", 10, 24),
    *both("avd_cl_conv_dgrad", "R5", 14, 10),
    *both("avd_cl_conv_wgrad", "R1", 12, 20), *both("avd_cl_conv_wgrad", "R2", 8, 20),
    *both("avd_cl_conv_wgrad", "R3", 16, 48), *both("avd_cl_conv_wgrad", "R3", 16, 112),
    *both("avd_cl_conv_wgrad", "R4", 10, 24), *both("avd_cl_conv_wgrad", "R5", 14, 10),
    # BN -> ReLU -> pool forward (modes 0/1/2, codes) and backward (reduce, apply); case = channels
    *both("avd_cl_bn_block", 16, 12, 20), *both("avd_cl_bn_block", 8, 7, 10),
    *both("avd_cl_bn_bwd_reduce_pooled", 16, 12, 20),
    # the first-layer fused routes, bf16
    *both("avd_cl_bn_bwd_apply_wgrad", "R2", 8, 20), *both("avd_cl_bn_bwd_apply_wgrad", "R3", 16, 48),
    *both("avd_cl_bn_bwd_apply_wgrad", "R3", 16, 112),
    *both("avd_cl_c1_recompute", "R2", 8, 20), *both("avd_cl_c1_recompute", "R3", 16, 48),
    *both("avd_cl_c1_recompute", "R3", 16, 112),
    *both("avd_cl_c1r3_codes", "R2", 8, 20),
    # H == 28 with W <= 32 stages whole-sample tiles (c1w3.hip c1r3_tr), and only H == W == 28 goes
    # to c1s3.hip: 28x20 runs the 28-row tile's passes 0 / 1 that no square reaches, 20x28 the
    # 4-row tile with virtual columns
    *both("avd_cl_bn_bwd_apply_wgrad", "R2", 28, 20), *both("avd_cl_c1_recompute", "R2", 28, 20),
    *both("avd_cl_c1r3_codes", "R2", 28, 20),
    *both("avd_cl_c1_codes", "R3", 16, 48), *both("avd_cl_c1_gram", "R3", 16, 48),
    *both("avd_c3_conv_eval", "R4", 10, 24),
    # bf16 3x3 layers with Cin, Cout % 32 == 0 run on conv3.hip alone, which takes W <= 62 (f32: generic)
    ("avd_cl_conv_fwd", "R4", 8, 64, D), ("avd_cl_conv_dgrad", "R4", 8, 64, D),
    # one side at the served size, the other not: the sizing queries answer 0
    *both("avd_cl_layer_bwd_slabs", "A2", 56, 40, D),
    *both("avd_cl_stat_pivot", "A2", 56, 40, D), *both("avd_cl_stat_pivot", "A3", 28, 20, D),
    *both("avd_cl_c1r5_rows", "I1", 28, 20, D),
    *both("avd_mx_conv", "A2", 56, 40, D), *both("avd_mx_conv", "A3", 28, 20, D),
    # ... and the squares they are cut from are served (the queries are asked the right question)
    ("avd_cl_layer_bwd_slabs", "A2", 56, 56, S), ("avd_cl_stat_pivot", "A2", 56, 56, S),
    ("avd_cl_stat_pivot", "A3", 28, 28, S), ("avd_cl_c1r5_rows", "I1", 28, 28, S),
    ("avd_mx_conv", "A2", 56, 56, S), ("avd_mx_conv", "A3", 28, 28, S),
]
SQUARE = {"A2": (8, 16, 5, 2), "A3": (16, 32, 5, 2), "I1": (1, 32, 5, 2)}   # Cin, Cout, K, pad

# The first-layer routes' per-axis rules as include/avdino.h states them, at their edges (query
# only): Cout, K, pad, H, W, verdict.  rows = avd_cl_c1_recompute_rows (every pass),
# slabs = avd_cl_apply_wgrad_slabs.
ROUTE_LIMITS = {
    "rows": [
        (8, 5, 2, 16, 112, S), (8, 5, 2, 112, 16, S), (8, 5, 2, 16, 128, D), (8, 5, 2, 24, 48, D),
        (8, 5, 2, 48, 24, D), (8, 3, 1, 16, 48, D),
        (16, 3, 1, 8, 128, S), (16, 3, 1, 128, 8, S), (16, 3, 1, 8, 132, D), (16, 5, 2, 8, 20, D),
        (32, 3, 1, 8, 120, S), (32, 3, 1, 120, 8, S), (32, 3, 1, 8, 124, D), (32, 3, 1, 8, 128, D),
        (32, 3, 1, 8, 18, D), (32, 3, 1, 10, 20, D), (32, 3, 1, 28, 20, S), (32, 3, 1, 20, 28, S),
        (64, 3, 1, 8, 72, S), (64, 3, 1, 72, 8, S), (64, 3, 1, 8, 76, D), (64, 3, 1, 28, 32, D),
        (64, 3, 1, 28, 36, S), (64, 3, 1, 32, 28, S), (64, 5, 2, 8, 20, D),
        (32, 5, 2, 8, 96, S), (32, 5, 2, 96, 8, S), (32, 5, 2, 8, 100, D),
    ],
    "slabs": [
        (8, 5, 2, 16, 112, S), (8, 5, 2, 112, 16, S), (8, 5, 2, 16, 128, D), (8, 5, 2, 24, 48, D),
        (8, 5, 2, 48, 24, D),
        (16, 3, 1, 8, 126, S), (16, 3, 1, 8, 128, D), (32, 3, 1, 8, 126, S), (32, 3, 1, 128, 8, S),
        (32, 3, 1, 8, 128, D), (32, 3, 1, 8, 21, D), (32, 3, 1, 10, 20, D), (32, 3, 1, 4, 22, S),
        (64, 3, 1, 8, 64, S), (64, 3, 1, 64, 8, S), (64, 3, 1, 8, 66, D), (32, 5, 2, 8, 20, D),
    ],
}


def rows_of(entry, verdict=S):
    return [(c, h, w) for e, c, h, w, v in TABLE if e == entry and v == verdict]


def ids_of(entry):
    return [f"{c}-{h}x{w}" for c, h, w in rows_of(entry)]


@pytest.fixture(scope="module")
def ops():
    from avdino import ops as _ops
    return _ops


# ------------------------------------------------------------------ planted data, padded buffers
def planted(g, N, C, H, W, B, lo=-1.0, hi=1.0):
    """[N, C, H, W] float64: noise + a term rising with h + another falling with w; BN group g
    (samples g*B ..) scaled by 10^g."""
    x = g.uniform(lo, hi, (N, C, H, W))
    x = x + 0.5 * (np.arange(H) / H)[None, None, :, None] - 0.3 * (np.arange(W) / W)[None, None, None, :]
    for gi in range(N // B):
        x[gi * B:(gi + 1) * B] *= 10.0 ** gi
    return x


class Buf:
    """A device buffer over-allocated to `alloc` elements + TAIL, sentinel-filled; `t` is the view
    of its leading elements that the kernels are given."""

    def __init__(self, shape, alloc, dtype, data=None):
        n = int(np.prod(shape))
        self.n = n
        self.int = not dtype.is_floating_point
        self.full = torch.full((max(n, int(alloc)) + TAIL,), -1 if self.int else float("nan"),
                               device="cuda", dtype=dtype)
        self.t = self.full[:n].view(*shape)
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32)).view(*shape).to(dtype))

    def check(self, written=True):
        """the tail is untouched; the lead is fully written (or, written=False, untouched too)"""
        tail, lead = self.full[self.n:], self.full[:self.n]
        if self.int:       # routing code words: -1 (every nibble 15) is no valid code
            assert bool((tail == -1).all()), "sentinel tail touched"
            assert bool((lead == -1).all()) != written, "codes not fully written / touched by a declined call"
        else:
            assert bool(torch.isnan(tail.float()).all()), "sentinel tail touched"
            if written:
                assert not bool(torch.isnan(lead.float()).any()), "output not fully written"
            else:
                assert bool(torch.isnan(lead.float()).all()), "output touched by a declined call"


def sq(N, H, W, C):
    M = max(H, W)
    return N * M * M * C


def put(a, alloc, dtype):
    return Buf(a.shape, alloc, dtype, data=a)


def vec(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def rows3(q, H, W):
    """a row / slab count for the buffer: the library's answer for this map, padded to the most it
    answers for the transposed and the max(H, W)-square map"""
    M = max(H, W)
    return max(q(H, W), q(W, H), q(M, M))


def grp_rel(a, b, G):
    """worst per-group rel-L2 of [N, ...] arrays (group-major samples)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    B = a.shape[0] // G
    return max(rel(a[g * B:(g + 1) * B], b[g * B:(g + 1) * B]) for g in range(G))


def grel(a, b):
    a, b = a.to(F64).reshape(-1), b.to(F64).reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def layout(ops, w, dgrad, T):
    Co, Ci, K, _ = w.shape
    wk = torch.empty(ops.cl_weight_elems(Co, Ci, K, dgrad), device="cuda", dtype=T)
    ops.cl_weight_layout(vec(w), wk, dgrad)
    return wk


def conv_inputs(case, H, W, dt, seed):
    Cin, Cout, K, pad, N, B = CASES[case]
    g = np.random.default_rng(seed)
    x = planted(g, N, Cin, H, W, B)
    w = g.uniform(-1, 1, (Cout, Cin, K, K)) / np.sqrt(Cin * K * K)
    b = g.uniform(-0.1, 0.1, Cout).astype(np.float32)
    if dt == "bf16":
        x, w = bf(x), bf(w)
    return x.astype(np.float32), w.astype(np.float32), b


# ------------------------------------------------------------------ conv forward / dgrad / wgrad
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_conv_fwd"), ids=ids_of("avd_cl_conv_fwd"))
def test_rect_conv_fwd_stats(ops, case, H, W, dt):
    Cin, Cout, K, pad, N, B = CASES[case]
    G, T = N // B, DT[dt]
    x, w, b = conv_inputs(case, H, W, dt, 1000 * H + W)
    y_ref, _ = O.conv2d_fwd(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), pad)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    assert y_ref.shape == (N, Cout, Ho, Wo)
    R = ops.cl_stat_rows(Ho, Wo, B, K, Cin, Cout, T)
    assert R > 0, "served shape: the statistics row query answered 0"
    Ra = rows3(lambda h, w_: ops.cl_stat_rows(h, w_, B, K, Cin, Cout, T), Ho, Wo)
    wk = layout(ops, w, 0, T)
    xb = put(nhwc(x), sq(N, H, W, Cin), T)
    yb = Buf((N, Ho, Wo, Cout), sq(N, Ho, Wo, Cout), T)
    sb = Buf((Cout * G * R * 2,), Cout * G * Ra * 2, torch.float32)
    ops.cl_conv_fwd(xb.t, wk, vec(b), yb.t, sb.t, N, B, Cin, H, W, Cout, K, pad)
    torch.cuda.synchronize()
    yb.check(), sb.check(), xb.check()
    yh = nchw(host(yb.t))
    e = grp_rel(yh, y_ref, G)
    print(f"{case} {H}x{W} {dt}: y rel {e:.2e}")
    assert e < TOL[dt], e
    st = host(sb.t).reshape(Cout, G, R, 2).sum(2)                 # per (channel, group)
    ys = yh.reshape(G, B, Cout, Ho, Wo)                           # statistics of the stored values
    for gi in range(G):
        assert rel(st[:, gi, 0], ys[gi].sum((0, 2, 3))) < 1e-5
        assert rel(st[:, gi, 1], (ys[gi] ** 2).sum((0, 2, 3))) < 1e-5
    # avd_cl_conv_fwd_pv: only where avd_cl_stat_pivot says 1 -- nowhere off the squares; with a
    # pivot the entry point answers AVD_ERR_ARG before any launch (conv_cl.hip: the pivot check
    # stands above every route)
    assert not ops.cl_stat_pivot(Ho, Wo, B, K, Cin, Cout, T)
    y2 = Buf((N, Ho, Wo, Cout), sq(N, Ho, Wo, Cout), T)
    s2 = Buf((Cout * G * R * 2,), Cout * G * Ra * 2, torch.float32)
    pv = torch.zeros(Cout, device="cuda")
    from avdino._lib import lib
    rc = lib.avd_cl_conv_fwd_pv(ops.p(xb.t), ops.p(wk), ops.p(vec(b)), ops.p(pv), ops.p(y2.t), ops.p(s2.t),
                                ops.dtcode(xb.t), N, B, Cin, H, W, Cout, K, pad, ops.stream())
    torch.cuda.synchronize()
    assert rc == AVD_ERR_ARG, rc
    y2.check(written=False), s2.check(written=False)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_conv_dgrad"), ids=ids_of("avd_cl_conv_dgrad"))
def test_rect_conv_dgrad(ops, case, H, W, dt):
    Cin, Cout, K, pad, N, B = CASES[case]
    T = DT[dt]
    x, w, _ = conv_inputs(case, H, W, dt, 1000 * H + W + 1)
    _, win = O.conv2d_fwd(x.astype(np.float64), w.astype(np.float64), np.zeros(Cout), pad)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    dy = planted(np.random.default_rng(5), N, Cout, Ho, Wo, B)
    dy = (bf(dy) if dt == "bf16" else dy).astype(np.float32)
    dx_ref, _, _ = O.conv2d_bwd(dy.astype(np.float64), win, w.astype(np.float64), x.shape, pad)
    wd = layout(ops, w, 1, T)
    dyb = put(nhwc(dy), sq(N, Ho, Wo, Cout), T)
    dxb = Buf((N, H, W, Cin), sq(N, H, W, Cin), T)
    ops.cl_conv_dgrad(dyb.t, wd, dxb.t, N, Cin, H, W, Cout, K, pad)
    torch.cuda.synchronize()
    dxb.check(), dyb.check()
    e = grp_rel(nchw(host(dxb.t)), dx_ref, N // B)
    print(f"{case} {H}x{W} {dt}: dx rel {e:.2e}")
    assert e < TOL[dt], e


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_conv_wgrad"), ids=ids_of("avd_cl_conv_wgrad"))
def test_rect_conv_wgrad(ops, case, H, W, dt):
    Cin, Cout, K, pad, N, B = CASES[case]
    T = DT[dt]
    x, _, _ = conv_inputs(case, H, W, dt, 1000 * H + W + 2)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    dy = planted(np.random.default_rng(6), N, Cout, Ho, Wo, B)
    dy = (bf(dy) if dt == "bf16" else dy).astype(np.float32)
    wz = np.zeros((Cout, Cin, K, K))
    _, win = O.conv2d_fwd(x.astype(np.float64), wz, np.zeros(Cout), pad)
    _, dw_ref, _ = O.conv2d_bwd(dy.astype(np.float64), win, wz, x.shape, pad)
    nch = ops.cl_wgrad_chunks(N, Cout, Cin, K)
    assert nch > 0
    per = Cout * Cin * K * K
    xb, dyb = put(nhwc(x), sq(N, H, W, Cin), T), put(nhwc(dy), sq(N, Ho, Wo, Cout), T)
    pb = Buf((nch * per,), nch * per, torch.float32)
    ops.cl_conv_wgrad(xb.t, dyb.t, pb.t, N, Cin, H, W, Cout, K, pad)
    dw = torch.empty(Cout, Cin, K, K, device="cuda")
    ops.sum_rows(pb.t, nch, per, dw)
    torch.cuda.synchronize()
    pb.check(), xb.check(), dyb.check()
    # operands are exact in both types; only the fp32 accumulation order differs
    e = rel(host(dw), dw_ref)
    print(f"{case} {H}x{W} {dt}: dw rel {e:.2e}")
    assert e < 1e-5, e


# ------------------------------------------------------------------ BN -> ReLU -> pool block
def _windows(a):
    """[N, H, W, C] -> [N, Hp, Wp, C, 4] in window order (0,0), (0,1), (1,0), (1,1), floor mode"""
    Hp, Wp = a.shape[1] // 2, a.shape[2] // 2
    a = a[:, :2 * Hp, :2 * Wp]
    return torch.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]], -1)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C,H,W", rows_of("avd_cl_bn_block"), ids=ids_of("avd_cl_bn_block"))
def test_rect_bn_block_fwd_bwd(ops, C, H, W, mode, dt):
    """tests/test_gpu_cl.py test_cl_bn_block_fwd_bwd with H != W (floor pooling of 7x10 / 10x7 to
    3x5 / 5x3), plus the routing codes of avd_cl_bn_relu_pool_codes (bf16, mode 0)."""
    G, B = 2, 2
    N, T = G * B, DT[dt]
    g = np.random.default_rng(H * 1000 + W * 10 + mode)
    y = planted(g, N, C, H, W, B, -2.0, 2.0) + 0.3
    y = (bf(y) if dt == "bf16" else y).astype(np.float32)
    gamma = (1 + g.uniform(-0.2, 0.2, C)).astype(np.float32)
    beta = g.uniform(-0.2, 0.2, C).astype(np.float32)
    z, bnc, _ = O.bn_train_fwd(y.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64), G, (2, 3))
    pmap, pc = O.maxpool2_fwd(np.maximum(z, 0))
    Hp, Wp = H // 2, W // 2
    assert pmap.shape == (N, C, Hp, Wp)
    out_ref = {0: pmap, 1: pmap.mean((2, 3)), 2: pmap.reshape(N, -1)}[mode]
    gout = g.uniform(-1, 1, out_ref.shape).astype(np.float32)
    if mode == 0 and dt == "bf16":
        gout = bf(gout)
    if mode == 0:
        dp = gout.astype(np.float64)
    elif mode == 1:
        dp = np.broadcast_to(gout[:, :, None, None] / (Hp * Wp), pmap.shape)
    else:
        dp = gout.reshape(pmap.shape).astype(np.float64)
    dz = O.maxpool2_bwd(dp, pc) * (z > 0)
    dy_ref, dg_ref, db_ref = O.bn_train_bwd(dz, bnc)

    y64 = y.astype(np.float64).reshape(G, B, C, -1).transpose(2, 0, 1, 3)
    parts = np.stack([y64.sum(-1), (y64 ** 2).sum(-1)], -1)          # [C][G][R = B][2]
    st = torch.empty(4, G * C, device="cuda")
    ops.bn_finalize(vec(parts), G, B, C, B * H * W, vec(gamma), vec(beta), st[0], st[1], st[2], st[3])
    yb = put(nhwc(y), sq(N, H, W, C), T)
    M2 = max(H, W) // 2
    if mode == 0:
        ob = Buf((N, Hp, Wp, C), N * M2 * M2 * C, T)
    else:
        ob = Buf(out_ref.shape, N * C * M2 * M2, torch.float32)
    ops.cl_bn_relu_pool(yb.t, st[2], st[3], ob.t, mode, N, B, C, H, W)
    torch.cuda.synchronize()
    ob.check(), yb.check()
    oh = nchw(host(ob.t)) if mode == 0 else host(ob.t)
    assert grp_rel(oh, out_ref, G) < (4e-3 if (dt == "bf16" and mode == 0) else 1e-5)

    if mode == 0 and dt == "bf16":
        o2 = Buf((N, Hp, Wp, C), N * M2 * M2 * C, T)
        cb = Buf((N * Hp * Wp * C // 8,), N * M2 * M2 * C // 8, torch.int32)
        ops.cl_bn_relu_pool_codes(yb.t, st[2], st[3], o2.t, cb.t, N, B, C, H, W)
        torch.cuda.synchronize()
        o2.check(), cb.check()
        assert torch.equal(o2.t, ob.t)
        cw = cb.t.view(N, Hp, Wp, C // 8, 1).to(torch.int64) & 0xFFFFFFFF
        nib = ((cw >> (4 * torch.arange(8, device="cuda"))) & 15).reshape(N, Hp, Wp, C)
        assert int(nib.max()) <= 4
        assert torch.equal(nib == 0, ob.t == 0)
        # the oracle's first-max argmax (row-major window order) wherever the window routes; the
        # window values are recomputed in float64 from the device's scale / shift and compared in
        # f32 (the kernel's one fmaf), as tests/test_gpu_lbwd_codes.py does
        sc = st[2].double().view(G, 1, 1, 1, C).expand(G, B, H, W, C).reshape(N, H, W, C)
        sf = st[3].double().view(G, 1, 1, 1, C).expand(G, B, H, W, C).reshape(N, H, W, C)
        a = torch.relu(yb.t.double() * sc + sf).to(torch.float32)
        win = _windows(a)
        best = win.max(-1).values
        first = (win == best.unsqueeze(-1)).to(torch.int64).argmax(-1)     # first maximum
        assert torch.equal(torch.where(best > 0, first + 1, torch.zeros_like(first)), nib)
        # ... which is the float64 oracle's argmax wherever its top two are not within f32 noise
        arg64 = torch.from_numpy(pc[0]).cuda().permute(0, 2, 3, 1)
        top2 = win.double().topk(2, -1).values
        clear = (best > 0) & ((top2[..., 0] - top2[..., 1]) > 1e-5 * top2[..., 0].abs())
        assert bool(clear.float().mean() > 0.5)
        assert torch.equal((nib - 1)[clear], arg64[clear])

    gb = put(nhwc(gout), N * M2 * M2 * C, T) if mode == 0 else put(gout, N * C * M2 * M2, torch.float32)
    R = ops.cl_bn_bwd_rows(B, C, H, W, T)
    assert R > 0
    Ra = rows3(lambda h, w_: ops.cl_bn_bwd_rows(B, C, h, w_, T), H, W)
    pb = Buf((C * G * R * 2,), C * G * Ra * 2, torch.float32)
    ops.cl_bn_bwd_reduce(yb.t, gb.t, mode, st[2], st[3], st[0], st[1], pb.t, N, B, C, H, W)
    torch.cuda.synchronize()
    pb.check()
    coef = torch.empty(G * C * 3, device="cuda")
    dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ops.bn_bwd_finalize(pb.t, G, R, C, B * H * W, vec(gamma), st[0], st[1], coef, dgam, dbet, None)
    assert rel(host(dgam), dg_ref) < 1e-5
    assert rel(host(dbet), db_ref) < 1e-5
    dyb = Buf((N, H, W, C), sq(N, H, W, C), T)
    ops.cl_bn_bwd_apply(yb.t, gb.t, mode, st[2], st[3], coef, dyb.t, N, B, C, H, W)
    torch.cuda.synchronize()
    dyb.check(), gb.check(), yb.check()
    assert grp_rel(nchw(host(dyb.t)), dy_ref, G) < (5e-3 if dt == "bf16" else 1e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("C,H,W", rows_of("avd_cl_bn_bwd_reduce_pooled"),
                         ids=ids_of("avd_cl_bn_bwd_reduce_pooled"))
def test_rect_bn_bwd_reduce_pooled(ops, C, H, W, mode, dt):
    """tests/test_gpu_cl.py test_bn_bwd_reduce_pooled_matches_y_path with H != W (incl. its
    gamma == 0 channel), and both kernels' dgamma / dbeta against the float64 oracle."""
    G, B = 2, 2
    N, T = G * B, DT[dt]
    g = np.random.default_rng(H * 31 + W + mode)
    y = planted(g, N, C, H, W, B, -2.0, 2.0)
    y = (bf(y) if dt == "bf16" else y).astype(np.float32)
    gamma = g.uniform(0.5, 1.5, C).astype(np.float32)
    gamma[1] = 0.0
    beta = (g.normal(size=C) * 0.1).astype(np.float32)
    z, bnc, stats = O.bn_train_fwd(y.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64), G, (2, 3))
    mean = stats[0].astype(np.float32)
    invstd = (1.0 / np.sqrt(stats[1] + O.BN_EPS)).astype(np.float32)
    scale = gamma[None] * invstd
    shift = beta[None] - mean * scale
    Hp, Wp, M2 = H // 2, W // 2, max(H, W) // 2
    yb = put(nhwc(y), sq(N, H, W, C), T)
    pshape = (N, Hp, Wp, C) if mode == 0 else (N * C * Hp * Wp,)
    PT = T if mode == 0 else torch.float32
    pool = Buf(pshape, N * M2 * M2 * C, PT)
    gout = g.normal(size=(N, C, Hp, Wp)).astype(np.float32)
    if mode == 0 and dt == "bf16":
        gout = bf(gout)
    gb = put(nhwc(gout) if mode == 0 else gout.reshape(-1), N * M2 * M2 * C, PT)
    dsc, dsf, dmu, div = vec(scale), vec(shift), vec(mean), vec(invstd)
    ops.cl_bn_relu_pool(yb.t, dsc, dsf, pool.t, mode, N, B, C, H, W)
    R = ops.cl_bn_bwd_rows(B, C, H, W, T)
    Ra = rows3(lambda h, w_: ops.cl_bn_bwd_rows(B, C, h, w_, T), H, W)
    p0 = Buf((C * G * R * 2,), C * G * Ra * 2, torch.float32)
    p1 = Buf((C * G * R * 2,), C * G * Ra * 2, torch.float32)
    ops.cl_bn_bwd_reduce(yb.t, gb.t, mode, dsc, dsf, dmu, div, p0.t, N, B, C, H, W)
    ops.cl_bn_bwd_reduce_pooled(yb.t, pool.t, gb.t, mode, vec(gamma), vec(beta), dmu, div, p1.t, N, B, C, H, W)
    torch.cuda.synchronize()
    p0.check(), p1.check(), pool.check(), gb.check(), yb.check()
    s0 = host(p0.t).reshape(C, G, R, 2).sum(2)
    s1 = host(p1.t).reshape(C, G, R, 2).sum(2)
    assert np.allclose(s1[..., 0], s0[..., 0], rtol=1e-5, atol=1e-4)     # sum dz: identical routing
    tol = 2e-6 if dt == "f32" else 4e-3                                  # bf16: rounding of p
    assert rel(s1[..., 1], s0[..., 1]) < tol
    # the y-path sums against the float64 oracle (f32 reductions: 1e-5)
    _, pc = O.maxpool2_fwd(np.maximum(z, 0))
    dz = O.maxpool2_bwd(gout.astype(np.float64), pc) * (z > 0)
    xhat = bnc[0].reshape(N, C, H, W)
    ref1 = dz.reshape(G, B, C, -1).sum((1, 3)).T
    ref2 = (dz * xhat).reshape(G, B, C, -1).sum((1, 3)).T
    ok = gamma != 0                    # gamma == 0: every z ties, the first pixel routes by rule
    assert rel(s0[ok, :, 0], ref1[ok]) < 1e-5
    assert rel(s0[ok, :, 1], ref2[ok]) < 1e-5


# ------------------------------------------------------------------ first-layer fused routes (bf16)
def _first_layer(case, H, W, seed):
    Cin, C, K, pad, N, B = CASES[case]
    assert Cin == 1
    g = np.random.default_rng(seed)
    x = bf(planted(g, N, 1, H, W, B, 0.0, 1.0))                      # [N, 1, H, W]
    w = bf(g.uniform(-1, 1, (C, 1, K, K)) / K)
    b = g.uniform(-0.1, 0.1, C).astype(np.float32)
    return g, x, w, b


def _taps(x, K, pad):
    """[N, 1, H, W] -> sliding windows [N, H, W, K*K] float64 (zero halo)"""
    win = np.lib.stride_tricks.sliding_window_view(
        np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad))), (K, K), (2, 3))
    return win[:, 0].reshape(x.shape[0], x.shape[2], x.shape[3], K * K)


@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_bn_bwd_apply_wgrad"), ids=ids_of("avd_cl_bn_bwd_apply_wgrad"))
def test_rect_bn_bwd_apply_wgrad(ops, case, H, W):
    """tests/test_gpu_cl.py test_cl_bn_bwd_apply_wgrad_fused_first_layer with H != W."""
    _, C, K, pad, N, B = CASES[case]
    G, T = N // B, BF
    g, x, _, _ = _first_layer(case, H, W, H * 7 + W)
    y = bf(planted(g, N, C, H, W, B, -1.5, 1.5) + 0.2)
    Hp, Wp, M2 = H // 2, W // 2, max(H, W) // 2
    gout = bf(g.uniform(-1, 1, (N, Hp, Wp, C)))
    scale = g.uniform(0.5, 1.5, G * C).astype(np.float32)
    shift = g.uniform(-0.3, 0.3, G * C).astype(np.float32)
    coef = g.uniform(-0.5, 0.5, G * C * 3).astype(np.float32)
    yb, xb = put(nhwc(y), sq(N, H, W, C), T), put(nhwc(x), sq(N, H, W, 1), T)
    gb = put(gout, N * M2 * M2 * C, T)
    dyb = Buf((N, H, W, C), sq(N, H, W, C), T)
    ops.cl_bn_bwd_apply(yb.t, gb.t, 0, vec(scale), vec(shift), vec(coef), dyb.t, N, B, C, H, W)
    nch = ops.cl_wgrad_chunks(N, C, 1, K)
    parts = torch.empty(nch * C * K * K, device="cuda")
    ops.cl_conv_wgrad(xb.t, dyb.t, parts, N, 1, H, W, C, K, pad)
    dw_ref = torch.empty(C, 1, K, K, device="cuda")
    ops.sum_rows(parts, nch, C * K * K, dw_ref)
    ns = ops.cl_apply_wgrad_slabs(T, N, 1, H, W, C, K, pad)
    assert ns > 0, "served shape: the slab query answered 0"
    na = rows3(lambda h, w_: ops.cl_apply_wgrad_slabs(T, N, 1, h, w_, C, K, pad), H, W)
    fb = Buf((ns * C * K * K,), na * C * K * K, torch.float32)
    ops.cl_bn_bwd_apply_wgrad(yb.t, gb.t, vec(scale), vec(shift), vec(coef), xb.t, fb.t, N, B, 1, H, W, C, K, pad)
    dw = torch.empty(C, 1, K, K, device="cuda")
    ops.sum_rows(fb.t, ns, C * K * K, dw)
    torch.cuda.synchronize()
    fb.check(), dyb.check(), yb.check(), xb.check(), gb.check()
    assert rel(host(dw), host(dw_ref)) < 1e-5, rel(host(dw), host(dw_ref))
    dw64 = np.einsum("nhwo,nhwt->ot", host(dyb.t), _taps(x, K, pad))     # float64, the same bf16 dy
    assert rel(host(dw), dw64) < 1e-5


def _pool_route(z, gz):
    """float64 dz [G, B, H, W, C] of the pooled gradient gz routed to the first max of z (relu'd
    BN output, [G, B, H, W, C]) where that max is > 0"""
    G, B, H, W, C = z.shape
    Hp, Wp = H // 2, W // 2
    zw = z.reshape(G, B, Hp, 2, Wp, 2, C).transpose(0, 1, 2, 4, 6, 3, 5).reshape(G, B, Hp, Wp, C, 4)
    am, best = zw.argmax(-1), zw.max(-1)
    dzw = np.where((np.arange(4) == am[..., None]) & (best[..., None] > 0), gz[..., None], 0.0)
    return dzw.reshape(G, B, Hp, Wp, C, 2, 2).transpose(0, 1, 2, 5, 3, 6, 4).reshape(G, B, H, W, C)


@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_c1_recompute"), ids=ids_of("avd_cl_c1_recompute"))
def test_rect_c1_recompute_passes(ops, case, H, W):
    """tests/test_gpu_cl.py test_cl_c1_recompute_passes_match_stored_y_path with H != W: passes
    0-4 and avd_cl_c1_recompute_combine against the stored-y chain (pooled map bit for bit) and
    float64."""
    _, C, K, pad, N, B = CASES[case]
    G, T, KK = N // B, BF, K * K
    Hp, Wp, M2 = H // 2, W // 2, max(H, W) // 2
    g, x, w, b = _first_layer(case, H, W, H + C + K + 100 * W)
    xb, tb = put(nhwc(x), sq(N, H, W, 1), T), vec(b)
    wk = layout(ops, w, 0, T)
    args = (N, B, 1, H, W, C, K, pad)

    def q(pas):
        r = ops.cl_c1_recompute_rows(pas, T, *args)
        assert r > 0, f"served shape: pass {pas} rows answered 0"
        return r, rows3(lambda h, w_: ops.cl_c1_recompute_rows(pas, T, N, B, 1, h, w_, C, K, pad), H, W)
    # stored-y path
    y = torch.empty(N, H, W, C, device="cuda", dtype=T)
    R0 = ops.cl_stat_rows(H, W, B, K, 1, C, T)
    st0 = torch.empty(C * G * R0 * 2, device="cuda")
    ops.cl_conv_fwd(xb.t, wk, tb, y, st0, *args)
    R1, R1a = q(ops.C1_STATS)
    s1b = Buf((C * G * R1 * 2,), C * G * R1a * 2, torch.float32)
    ops.cl_c1_recompute(ops.C1_STATS, xb.t, wk, tb, *args, out=s1b.t)
    torch.cuda.synchronize()
    s1b.check()
    s0 = host(st0).reshape(C, G, R0, 2).sum(2)
    s1 = host(s1b.t).reshape(C, G, R1, 2).sum(2)
    assert rel(s1, s0) < 1e-6
    gamma = (1 + g.uniform(-.2, .2, C)).astype(np.float32)
    beta = g.uniform(-.2, .2, C).astype(np.float32)
    bn = torch.empty(4, G * C, device="cuda")
    ops.bn_finalize(st0, G, R0, C, B * H * W, vec(gamma), vec(beta), bn[0], bn[1], bn[2], bn[3])
    z0 = torch.empty(N, Hp, Wp, C, device="cuda", dtype=T)
    ops.cl_bn_relu_pool(y, bn[2], bn[3], z0, 0, N, B, C, H, W)
    z1 = Buf((N, Hp, Wp, C), N * M2 * M2 * C, T)
    ops.cl_c1_recompute(ops.C1_APPLY, xb.t, wk, tb, *args, scale=bn[2], shift=bn[3], z=z1.t)
    torch.cuda.synchronize()
    z1.check()
    assert torch.equal(z0, z1.t)
    gzh = bf(g.uniform(-1, 1, (N, Hp, Wp, C)))
    gzb = put(gzh, N * M2 * M2 * C, T)
    gz = gzb.t
    Rb = ops.cl_bn_bwd_rows(B, C, H, W, T)
    p0 = torch.empty(C * G * Rb * 2, device="cuda")
    ops.cl_bn_bwd_reduce(y, gz, 0, bn[2], bn[3], bn[0], bn[1], p0, N, B, C, H, W)
    Rr, Rra = q(ops.C1_REDUCE)
    p1 = Buf((C * G * Rr * 2,), C * G * Rra * 2, torch.float32)
    ops.cl_c1_recompute(ops.C1_REDUCE, xb.t, wk, tb, *args, scale=bn[2], shift=bn[3], mean=bn[0],
                        invstd=bn[1], gz=gz, out=p1.t)
    torch.cuda.synchronize()
    p1.check()
    r0 = host(p0).reshape(C, G, Rb, 2).sum(2)
    r1 = host(p1.t).reshape(C, G, Rr, 2).sum(2)
    assert rel(r1, r0) < 1e-5, rel(r1, r0)
    coef = torch.empty(G * C * 3, device="cuda")
    dg, dbt = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ops.bn_bwd_finalize(p0, G, Rb, C, B * H * W, vec(gamma), bn[0], bn[1], coef, dg, dbt, None)
    ns = ops.cl_apply_wgrad_slabs(T, N, 1, H, W, C, K, pad)
    assert ns > 0
    f0 = torch.empty(ns * C * KK, device="cuda")       # the stored-y fused apply + wgrad (c1p8 / c1w3)
    ops.cl_bn_bwd_apply_wgrad(y, gz, bn[2], bn[3], coef, xb.t, f0, *args)
    nw, nwa = q(ops.C1_WGRAD)
    f1 = Buf((nw * C * KK,), nwa * C * KK, torch.float32)
    ops.cl_c1_recompute(ops.C1_WGRAD, xb.t, wk, tb, *args, scale=bn[2], shift=bn[3], coef=coef, gz=gz, out=f1.t)
    torch.cuda.synchronize()
    f1.check()
    d0, d1 = torch.empty(C * KK, device="cuda"), torch.empty(C * KK, device="cuda")
    ops.sum_rows(f0, ns, C * KK, d0)
    ops.sum_rows(f1.t, nw, C * KK, d1)
    assert rel(host(d1), host(d0)) < 1e-6
    # pass 4: the reduce rows of pass 2 plus the moments; dW = combine(moments, coef)
    R4, R4a = q(ops.C1_REDUCE_MOMENTS)
    mc = ops.c1_moment_cols(C, K)
    m4 = Buf((C * G * R4 * 2 + R4 * G * mc,), C * G * R4a * 2 + R4a * G * mc, torch.float32)
    ops.cl_c1_recompute(ops.C1_REDUCE_MOMENTS, xb.t, wk, tb, *args, scale=bn[2], shift=bn[3], mean=bn[0],
                        invstd=bn[1], gz=gz, out=m4.t)
    torch.cuda.synchronize()
    m4.check(), xb.check(), gzb.check()
    r4 = host(m4.t[:C * G * R4 * 2]).reshape(C, G, R4, 2).sum(2)
    assert rel(r4, r0) < 1e-5, rel(r4, r0)
    mom = torch.empty(G * mc, device="cuda")
    ops.sum_rows(m4.t, R4, G * mc, mom, off=C * G * R4 * 2)
    mh = host(mom).reshape(G, mc)
    xk = _taps(x, K, pad).reshape(G, B, H, W, KK)
    gram = np.einsum("gbhwi,gbhwj->gij", xk, xk)
    if C != 8:   # c1r3 layout: Gram rows with the ones tap [KK][KK + 1]
        gk = mh[:, C * KK:].reshape(G, KK, KK + 1)[:, :, :KK]
        sk = mh[:, C * KK:].reshape(G, KK, KK + 1)[:, :, KK]
    else:
        gk, sk = mh[:, C * KK:C * KK + KK * KK].reshape(G, KK, KK), mh[:, C * KK + KK * KK:]
    for gi in range(G):
        assert rel(gk[gi], gram[gi]) < 1e-5, rel(gk[gi], gram[gi])
        assert rel(sk[gi], xk[gi].sum((0, 1, 2))) < 1e-5
    dk = torch.empty(C * KK, device="cuda")
    ops.cl_c1_recompute_combine(mom, coef, wk, tb, dk, G, C, K)
    yb_ = host(y).reshape(G, B, H, W, C)
    zr = np.maximum(yb_ * host(bn[2]).reshape(G, 1, 1, 1, C) + host(bn[3]).reshape(G, 1, 1, 1, C), 0)
    dz = _pool_route(zr, gzh.astype(np.float64).reshape(G, B, Hp, Wp, C))
    mz = np.einsum("gbhwc,gbhwt->gct", dz, xk)
    for gi in range(G):
        assert rel(mh[gi, :C * KK].reshape(C, KK), mz[gi]) < 1e-5
    yex = np.einsum("gbhwt,ct->gbhwc", xk, w.reshape(C, KK).astype(np.float64)) + b.astype(np.float64)
    k3 = host(coef).reshape(G, 1, 1, 1, C, 3)
    dy64 = k3[..., 0] * dz + k3[..., 1] * yex + k3[..., 2]
    dw64 = np.einsum("gbhwc,gbhwt->ct", dy64, xk)
    e64 = rel(host(dk), dw64.reshape(-1))
    err = rel(host(dk), host(d0))
    print("pass-4 dW rel: vs float64", e64, "vs stored-y path", err)
    assert e64 < 1e-4, e64
    assert err < 1e-2, err


def _routed_family(ops, fam, case, H, W):
    """The code-routed first-layer backward (fam "c1": avd_cl_c1_apply_codes / _moments_codes /
    _codes_combine, the 5x5 1 -> 8 audio layer; "c1r3": the avd_cl_c1r3_* 3x3 1 -> 32 layer) as
    tests/test_gpu_benchsize.py test_conv1_routed_backward_bench_size and
    tests/test_gpu_c1r3_codes.py test_conv1_3x3_routed_backward check it, with H != W."""
    _, C, K, pad, N, B = CASES[case]
    G, T, KK = N // B, BF, K * K
    Hp, Wp, M2 = H // 2, W // 2, max(H, W) // 2
    g, xh, wh, bh = _first_layer(case, H, W, 23 + H + 50 * W)
    xb = put(nhwc(xh), sq(N, H, W, 1), T)
    x, bias = xb.t, vec(bh)
    wk = layout(ops, wh, 0, T)
    args = (N, B, 1, H, W, C, K, pad)
    y = torch.empty(N, H, W, C, device="cuda", dtype=T)
    R0 = ops.cl_stat_rows(H, W, B, K, 1, C, T)
    st0 = torch.empty(C * G * R0 * 2, device="cuda")
    ops.cl_conv_fwd(x, wk, bias, y, st0, *args)
    gamma, beta = vec(g.uniform(0.8, 1.2, C)), vec(g.uniform(-0.2, 0.2, C))
    bn = torch.empty(4, G * C, device="cuda")
    ops.bn_finalize(st0, G, R0, C, B * H * W, gamma, beta, bn[0], bn[1], bn[2], bn[3])
    z0 = torch.empty(N, Hp, Wp, C, device="cuda", dtype=T)
    ops.cl_bn_relu_pool(y, bn[2], bn[3], z0, 0, N, B, C, H, W)
    z1 = torch.full_like(z0, float("nan"))
    ops.cl_c1_recompute(ops.C1_APPLY, x, wk, bias, *args, scale=bn[2], shift=bn[3], z=z1)
    z2 = Buf((N, Hp, Wp, C), N * M2 * M2 * C, T)
    if fam == "c1":
        codes = Buf((N * Hp * Wp,), N * M2 * M2, torch.int32)
        ops.c1_apply_codes(x, wk, bias, bn[2], bn[3], z2.t, codes.t, N, B, H, W)
        Rc, mc = ops.c1_codes_rows(N, B, H, W), ops.c1_codes_cols()
        Ra = rows3(lambda h, w_: ops.c1_codes_rows(N, B, h, w_), H, W)
    else:
        codes = Buf((N * Hp * Wp * C // 4,), N * M2 * M2 * C // 4, torch.int16)
        ops.c1r3_apply_codes(x, wk, bias, bn[2], bn[3], z2.t, codes.t, N, B, H, W, C)
        Rc, mc = ops.c1r3_codes_rows(N, B, H, W, C), ops.c1r3_codes_cols(C)
        Ra = rows3(lambda h, w_: ops.c1r3_codes_rows(N, B, h, w_, C), H, W)
    torch.cuda.synchronize()
    z2.check(), codes.check()
    assert torch.equal(z1, z2.t) and torch.equal(z0, z2.t)
    assert Rc > 0 and mc == C * KK + KK * KK + KK + C
    gzb = put(bf(g.uniform(-1, 1, (N, Hp, Wp, C))), N * M2 * M2 * C, T)
    gz = gzb.t
    parts = Buf((Rc * G * mc,), Ra * G * mc, torch.float32)
    if fam == "c1":
        ops.c1_moments_codes(x, gz, codes.t, parts.t, N, B, H, W)
    else:
        ops.c1r3_moments_codes(x, wk, gz, codes.t, parts.t, N, B, H, W, C)
    torch.cuda.synchronize()
    parts.check(), xb.check(), gzb.check()
    mom = torch.empty(G * mc, device="cuda")
    ops.sum_rows(parts.t, Rc, G * mc, mom)
    dw = torch.empty(C * KK, device="cuda")
    dg, db, dbi = (torch.empty(C, device="cuda") for _ in range(3))
    coef = torch.empty(G * C * 3, device="cuda")
    if fam == "c1":
        ops.c1_codes_combine(mom, wk, bias, gamma, bn[0], bn[1], B * H * W, dw, dg, db, dbi, coef, G)
    else:
        ops.c1r3_codes_combine(mom, wk, bias, gamma, bn[0], bn[1], B * H * W, dw, dg, db, dbi, coef, G, C)
    # float64 from the same routing (first max of relu(bn(y)) of the stored bf16 y)
    u = F.unfold(x.permute(0, 3, 1, 2).to(F64), K, padding=pad).view(G, B, KK, H * W)
    gram = torch.einsum("gbip,gbjp->gij", u, u)
    sx = u.sum((1, 3))
    sc, sf = bn[2].view(G, 1, 1, 1, C).to(F64), bn[3].view(G, 1, 1, 1, C).to(F64)
    zz = torch.relu(y.view(G, B, H, W, C).to(F64) * sc + sf)
    zw = zz.view(G * B, Hp, 2, Wp, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(G * B, Hp, Wp, C, 4)
    best, am = zw.max(-1)
    dzw = torch.where((torch.arange(4, device="cuda") == am[..., None]) & (best[..., None] > 0),
                      gz.to(F64)[..., None], torch.zeros((), device="cuda", dtype=F64))
    dz = dzw.view(G, B, Hp, Wp, C, 2, 2).permute(0, 1, 2, 5, 3, 6, 4).reshape(G, B, H * W, C)
    mz = torch.einsum("gbpc,gbtp->gct", dz, u)
    s1 = dz.sum((1, 2))
    mh = mom.view(G, mc).to(F64)
    for gi in range(G):       # per group: group 1 is 10x (its Gram 100x) group 0
        assert grel(mh[gi, :C * KK].view(C, KK), mz[gi]) < 1e-5
        assert grel(mh[gi, C * KK:C * KK + KK * KK].view(KK, KK), gram[gi]) < 1e-5
        assert grel(mh[gi, C * KK + KK * KK:C * KK + KK * KK + KK], sx[gi]) < 1e-5
        assert grel(mh[gi, C * KK + KK * KK + KK:], s1[gi]) < 1e-5
    w64 = torch.from_numpy(wh.reshape(C, KK)).cuda().to(F64)
    b64 = bias.to(F64)
    n = float(B * H * W)
    sy = torch.einsum("ct,gct->gc", w64, mz) + b64[None] * s1
    mu, iv, ga = bn[0].view(G, C).to(F64), bn[1].view(G, C).to(F64), gamma.to(F64)[None]
    s2 = (sy - mu * s1) * iv
    k1, kx, k0 = ga * iv, -ga * iv * iv * s2 / n, -ga * iv * s1 / n + ga * iv * iv * mu * s2 / n
    syg = torch.einsum("ct,gts->gcs", w64, gram) + b64[None, :, None] * sx[:, None, :]
    dw64 = (k1[..., None] * mz + kx[..., None] * syg + k0[..., None] * sx[:, None, :]).sum(0)
    k3 = coef.view(G, C, 3).to(F64)
    print(f"{fam} {H}x{W}: dW vs f64", grel(dw, dw64), "coef", grel(k3, torch.stack([k1, kx, k0], -1)))
    assert grel(k3, torch.stack([k1, kx, k0], -1)) < 1e-6
    assert grel(dg, s2.sum(0)) < 1e-5 and grel(db, s1.sum(0)) < 1e-5
    assert grel(dw, dw64) < 1e-5, grel(dw, dw64)
    # the recomputing moments pass (pass 4) on the same state
    R4 = ops.cl_c1_recompute_rows(ops.C1_REDUCE_MOMENTS, T, *args)
    mc4 = ops.c1_moment_cols(C, K)
    m4 = torch.empty(C * G * R4 * 2 + R4 * G * mc4, device="cuda")
    ops.cl_c1_recompute(ops.C1_REDUCE_MOMENTS, x, wk, bias, *args, scale=bn[2], shift=bn[3], mean=bn[0],
                        invstd=bn[1], gz=gz, out=m4)
    cf4 = torch.empty(G * C * 3, device="cuda")
    dg4, db4 = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ops.bn_bwd_finalize(m4, G, R4, C, B * H * W, gamma, bn[0], bn[1], cf4, dg4, db4, None)
    mom4 = torch.empty(G * mc4, device="cuda")
    ops.sum_rows(m4, R4, G * mc4, mom4, off=C * G * R4 * 2)
    d4 = torch.empty(C * KK, device="cuda")
    ops.cl_c1_recompute_combine(mom4, cf4, wk, bias, d4, G, C, K)
    assert grel(dw, d4) < 3e-3 and grel(db, db4) < 1e-5, (grel(dw, d4), grel(db, db4))


@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_c1r3_codes"), ids=ids_of("avd_cl_c1r3_codes"))
def test_rect_c1r3_routed_backward(ops, case, H, W):
    _routed_family(ops, "c1r3", case, H, W)


@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_c1_codes"), ids=ids_of("avd_cl_c1_codes"))
def test_rect_c1_routed_backward(ops, case, H, W):
    _routed_family(ops, "c1", case, H, W)


@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_c1_gram"), ids=ids_of("avd_cl_c1_gram"))
def test_rect_c1_gram_family(ops, case, H, W):
    """tests/test_gpu_c1_gram.py with H != W: avd_cl_c1_gram / _gram_finalize against float64 of
    the exact conv output (test_gram_stats, off = 0), then avd_cl_c1_moments_codes_ng +
    avd_cl_c1_codes_combine_gram against the full routed pass (test_split_backward_matches_full)."""
    _, C, K, pad, N, B = CASES[case]
    G, T = N // B, BF
    Hp, Wp, M2 = H // 2, W // 2, max(H, W) // 2
    g, xh, wh, bh = _first_layer(case, H, W, 29 + H + 50 * W)
    xb = put(nhwc(xh), sq(N, H, W, 1), T)
    x, bias = xb.t, vec(bh)
    gamma, beta = vec(g.uniform(0.8, 1.2, C)), vec(g.uniform(-0.2, 0.2, C))
    wk = layout(ops, wh, 0, T)
    R, gc, mc = ops.c1_codes_rows(N, B, H, W), ops.c1_gram_cols(), ops.c1_codes_cols()
    assert R > 0 and gc == 650
    Ra = rows3(lambda h, w_: ops.c1_codes_rows(N, B, h, w_), H, W)
    parts = Buf((R * G * max(gc, mc),), Ra * G * max(gc, mc), torch.float32)
    ops.c1_gram(x, parts.t, N, B, H, W)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(parts.t[:R * G * gc]).any()) and bool(torch.isnan(parts.full[R * G * gc:]).all())
    gram = torch.empty(G * gc, device="cuda")
    ops.sum_rows(parts.t, R, G * gc, gram)
    bn = torch.empty(4, G * C, device="cuda")
    rm0, rv0 = vec(g.uniform(0, 1, C)), vec(g.uniform(0.5, 1.5, C))
    rm, rv = rm0.clone(), rv0.clone()
    n = B * H * W
    ops.c1_gram_finalize(gram, wk, bias, gamma, beta, n, bn[0], bn[1], bn[2], bn[3], rm, rv, G)
    u = F.unfold(x.permute(0, 3, 1, 2).to(F64), K, padding=pad).view(G, B, 25, H * W)
    w64 = torch.from_numpy(wh.reshape(C, 25)).cuda().to(F64)
    y64 = torch.einsum("ct,gbtp->gbcp", w64, u) + bias.to(F64)[None, None, :, None]
    mean = y64.mean((1, 3))
    var = (y64 ** 2).mean((1, 3)) - mean * mean
    gh = gram.view(G, gc).double()
    for gi in range(G):
        assert grel(gh[gi, :625].view(25, 25), torch.einsum("bip,bjp->ij", u[gi], u[gi])) < 1e-6
        assert grel(gh[gi, 625:], u[gi].sum((0, 2))) < 1e-6
    iv = 1 / torch.sqrt(var + 1e-5)
    sc = gamma.double()[None] * iv
    sf = beta.double()[None] - mean * sc
    assert grel(bn[0].view(G, C), mean) < 1e-5
    assert grel(bn[1].view(G, C), iv) < 1e-5
    assert grel(bn[2].view(G, C), sc) < 1e-5
    assert grel(bn[3].view(G, C), sf) < 1e-5
    erm, erv = rm0.double(), rv0.double()
    for gi in range(G):
        erm = 0.9 * erm + 0.1 * mean[gi]
        erv = 0.9 * erv + 0.1 * var[gi] * n / (n - 1)
    assert grel(rm, erm) < 1e-5 and grel(rv, erv) < 1e-5
    # the split backward against the full routed pass, on the same codes
    z = Buf((N, Hp, Wp, C), N * M2 * M2 * C, T)
    codes = Buf((N * Hp * Wp,), N * M2 * M2, torch.int32)
    ops.c1_apply_codes(x, wk, bias, bn[2], bn[3], z.t, codes.t, N, B, H, W)
    gzb = put(bf(g.uniform(-1, 1, (N, Hp, Wp, C))), N * M2 * M2 * C, T)
    outs = []
    for split in (False, True):
        parts.full.fill_(float("nan"))
        (ops.c1_moments_codes_ng if split else ops.c1_moments_codes)(x, gzb.t, codes.t, parts.t, N, B, H, W)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(parts.t[:R * G * mc]).any()) and bool(torch.isnan(parts.full[R * G * mc:]).all())
        mom = torch.empty(G * mc, device="cuda")
        ops.sum_rows(parts.t, R, G * mc, mom)
        r = [torch.empty(C * 25, device="cuda")] + [torch.empty(C, device="cuda") for _ in range(3)]
        coef = torch.empty(G * C * 3, device="cuda")
        if split:
            ops.c1_codes_combine_gram(mom, gram, wk, bias, gamma, bn[0], bn[1], n, *r, coef, G)
        else:
            mh = mom.view(G, mc)
            assert grel(mh[:, C * 25:C * 25 + 650], gram.view(G, gc)) < 1e-6
            ops.c1_codes_combine(mom, wk, bias, gamma, bn[0], bn[1], n, *r, coef, G)
        outs.append(r + [coef])
    torch.cuda.synchronize()
    z.check(), xb.check(), gzb.check(), codes.check()
    for a, b_ in zip(*outs):
        assert grel(b_, a) < 1e-5 or (a - b_).abs().max() < 1e-6 * a.abs().max().clamp_min(1.0), grel(a, b_)


# ------------------------------------------------------------------ the fused eval-mode 3x3 layer
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case,H,W", rows_of("avd_c3_conv_eval"), ids=ids_of("avd_c3_conv_eval"))
def test_rect_c3_conv_eval(ops, case, H, W, mode):
    """tests/test_gpu_c3_eval.py with H != W: bit-identical to avd_cl_conv_fwd + avd_cl_bn_relu_pool,
    and the float64 band of test_c3_conv_eval_float64_sanity (the stored bf16 map's 5e-3; mode 1
    averages non-negative values each inside that band, so the same bound holds for it)."""
    C, Oc, K, pad, N, _ = CASES[case]
    Hp, Wp, M2 = H // 2, W // 2, max(H, W) // 2
    g = np.random.default_rng(100 + H)
    xh = bf(planted(g, N, C, H, W, N))
    wh = bf(g.uniform(-1, 1, (Oc, C, 3, 3)) / (3 * C ** 0.5))
    b = g.uniform(-0.1, 0.1, Oc).astype(np.float32)
    scale = g.uniform(0.5, 1.5, Oc).astype(np.float32)
    scale[1::2] *= -1                 # both signs
    scale[3] = 0.0                    # one exact zero channel
    shift = g.uniform(-0.3, 0.3, Oc).astype(np.float32)
    shift[5::8] = -50.0               # all-negative channels: pooled output all zero
    xb = put(nhwc(xh), sq(N, H, W, C), BF)
    wk = layout(ops, wh, 0, BF)
    db, dsc, dsf = vec(b), vec(scale), vec(shift)
    y = torch.empty(N, H, W, Oc, device="cuda", dtype=BF)
    ops.cl_conv_fwd(xb.t, wk, db, y, None, N, N, C, H, W, Oc, 3, 1)
    if mode == 0:
        ref = torch.empty(N, Hp, Wp, Oc, device="cuda", dtype=BF)
        out = Buf((N, Hp, Wp, Oc), N * M2 * M2 * Oc, BF)
    else:
        ref = torch.empty(N, Oc, device="cuda")
        out = Buf((N, Oc), N * Oc, torch.float32)
    ops.cl_bn_relu_pool(y, dsc, dsf, ref, mode, N, N, Oc, H, W)
    assert ops.c3_eval_serves(N, H, W, C, Oc, mode), "served shape: avd_c3_eval_serves answered 0"
    assert ops.c3_conv_eval(xb.t, wk, db, dsc, dsf, out.t, mode, N, H, W, C, Oc)
    torch.cuda.synchronize()
    out.check(), xb.check()
    assert torch.equal(out.t, ref), (out.t.float() - ref.float()).abs().max().item()
    assert bool((ref[..., 5::8] == 0).all())
    y64 = F.conv2d(torch.from_numpy(xh).double(), torch.from_numpy(wh).double(), torch.from_numpy(b).double(),
                   padding=1)
    y64 = y64.float().to(BF).double()
    z = torch.relu(y64 * torch.from_numpy(scale).double()[None, :, None, None]
                   + torch.from_numpy(shift).double()[None, :, None, None])
    r64 = F.max_pool2d(z, 2)
    r64 = r64.permute(0, 2, 3, 1) if mode == 0 else r64.mean((2, 3))
    err = grel(out.t.cpu(), r64)
    print(f"c3_conv_eval {H}x{W} mode {mode} vs float64: rel-L2 {err:.3e}")
    assert err < TOL["bf16"], err


# ------------------------------------------------------------------ the table: declines and limits
def _query(ops, entry, case, H, W):
    """the sizing queries of a TABLE row: all > 0 = served, all == 0 = declined"""
    from avdino._lib import lib
    Cin, Cout, K, pad = SQUARE[case]
    N, B = 8, 4
    if entry == "avd_cl_layer_bwd_slabs":
        return [ops.cl_layer_bwd_slabs(BF, N, Cin, H, W, Cout, K, pad)]
    if entry == "avd_cl_stat_pivot":
        return [int(ops.cl_stat_pivot(H, W, B, K, Cin, Cout, BF))]
    if entry == "avd_cl_c1r5_rows":
        return [ops.c1r5_codes_rows(N, B, H, W), ops.c1r5_stats_rows(N, B, H, W)]
    assert entry == "avd_mx_conv"
    return [lib.avd_mx_conv_serves(Cin, H, W, Cout, K, pad, 0), lib.avd_mx_conv_serves(Cin, H, W, Cout, K, pad, 1),
            lib.avd_mx_conv_ns(Cin, H, W, Cout, K, pad, 0), lib.avd_mx_conv_ns(Cin, H, W, Cout, K, pad, 1),
            lib.avd_mx_stat_rows(H, W, B, K, Cin, Cout, pad)]


@pytest.mark.parametrize("entry,case,H,W,verdict", [r for r in TABLE if r[1] in SQUARE],
                         ids=[f"{r[0]}-{r[1]}-{r[2]}x{r[3]}" for r in TABLE if r[1] in SQUARE])
def test_rect_sizing_queries(ops, entry, case, H, W, verdict):
    got = _query(ops, entry, case, H, W)
    if verdict == S:
        assert all(v > 0 for v in got), got
    else:
        assert all(v == 0 for v in got), got


@pytest.mark.parametrize("H,W", [(56, 40), (40, 56), (28, 20), (20, 28)])
def test_rect_mx_wgrad_declines(ops, H, W):
    """avd_mx_wgrad_chunks takes H alone (its ABI has no W): it answers for the H x H layer, so it
    is 0 when H is not the served size; avd_mx_conv_wgrad itself checks H != W first."""
    from avdino._lib import lib
    case = "A2" if 56 in (H, W) else "A3"
    Cin, Cout, K, pad = SQUARE[case]
    served = 56 if case == "A2" else 28
    N = 16
    ch = ops.mx_wgrad_chunks(N, Cin, H, Cout, K, pad)
    assert (ch > 0) == (H == served), ch
    x = Buf((N, H, W, Cin), sq(N, H, W, Cin), BF)
    dy = Buf((N, H, W, Cout), sq(N, H, W, Cout), BF)
    nsq = max(ops.mx_wgrad_chunks(N, Cin, served, Cout, K, pad), 1)
    parts = Buf((nsq * Cout * Cin * K * K,), nsq * Cout * Cin * K * K, torch.float32)
    rc = lib.avd_mx_conv_wgrad(ops.p(x.t), ops.p(dy.t), ops.p(parts.t), N, Cin, H, W, Cout, K, pad, ops.stream())
    torch.cuda.synchronize()
    assert rc == AVD_ERR_SHAPE, rc
    parts.check(written=False)


LAUNCHERS = ("avd_cl_layer_bwd_slabs", "avd_cl_c1r5_rows", "avd_mx_conv")


@pytest.mark.parametrize("entry,case,H,W", [r[:4] for r in TABLE if r[4] == D and r[0] in LAUNCHERS],
                         ids=[f"{r[0]}-{r[2]}x{r[3]}" for r in TABLE if r[4] == D and r[0] in LAUNCHERS])
def test_rect_declined_entry_points_launch_nothing(ops, entry, case, H, W):
    """The launching entry points whose host code checks the shape before the first launch
    (read in lbwd.hip lbwd_launch, c1r5.hip, conv_ws8.hip avd_mx_conv_fwd / _dgrad): they return
    AVD_ERR_SHAPE and leave the sentinel-filled outputs untouched."""
    from avdino._lib import lib
    Cin, Cout, K, pad = SQUARE[case]
    N, B = 8, 4
    G = N // B
    Hp, Wp, M = H // 2, W // 2, max(H, W)
    x = Buf((N, H, W, Cin), sq(N, H, W, Cin), BF)
    x.full.zero_()
    st = ops.stream()
    p = ops.p
    coefs = torch.ones(4, G * Cout * 3, device="cuda")
    if entry == "avd_cl_layer_bwd_slabs":
        y = torch.zeros(N * M * M * Cout, device="cuda", dtype=BF)
        wk_d = torch.zeros(ops.cl_weight_elems(Cout, Cin, K, 1), device="cuda", dtype=BF)
        slabs = ops.cl_layer_bwd_slabs(BF, N, Cin, M, M, Cout, K, pad)
        assert slabs > 0
        dx = Buf((N, H, W, Cin), sq(N, H, W, Cin), BF)
        parts = Buf((slabs * Cout * Cin * K * K,), slabs * Cout * Cin * K * K, torch.float32)
        codes = torch.zeros(N * M * M * Cout // 8, device="cuda", dtype=torch.int32)
        rc = [lib.avd_cl_layer_bwd(p(y), p(y), p(coefs[0]), p(coefs[1]), p(coefs[2]), None, p(x.t), p(wk_d),
                                   p(dx.t), p(parts.t), slabs, 1, N, B, Cin, H, W, Cout, K, pad, st),
              lib.avd_cl_layer_bwd_codes(p(y), p(y), p(codes), p(coefs[2]), p(x.t), p(wk_d), p(dx.t),
                                         p(parts.t), slabs, 1, N, B, Cin, H, W, Cout, K, pad, st)]
        outs = [dx, parts]
    elif entry == "avd_cl_c1r5_rows":
        wk = torch.zeros(ops.cl_weight_elems(Cout, 1, K, 0), device="cuda", dtype=BF)
        R = max(ops.c1r5_codes_rows(N, B, 28, 28), ops.c1r5_stats_rows(N, B, 28, 28))
        assert R > 0
        stats = Buf((Cout * G * R * 2,), Cout * G * R * 2, torch.float32)
        z = Buf((N, Hp, Wp, Cout), N * (M // 2) ** 2 * Cout, BF)
        codes = Buf((N * Hp * Wp * 8,), N * (M // 2) ** 2 * 8, torch.int16)
        mom = Buf((R * G * ops.c1r5_codes_cols(),), R * G * ops.c1r5_codes_cols(), torch.float32)
        gz = torch.zeros(N * (M // 2) ** 2 * Cout, device="cuda", dtype=BF)
        cz = torch.zeros(N * (M // 2) ** 2 * 8, device="cuda", dtype=torch.int16)
        rc = [lib.avd_cl_c1r5_stats(p(x.t), p(wk), None, p(stats.t), N, B, H, W, st),
              lib.avd_cl_c1r5_apply_codes(p(x.t), p(wk), None, p(coefs[0]), p(coefs[1]), p(z.t), p(codes.t),
                                          N, B, H, W, st),
              lib.avd_cl_c1r5_moments_codes(p(x.t), p(gz), p(cz), p(mom.t), N, B, H, W, st)]
        outs = [stats, z, codes, mom]
    else:
        wq = torch.zeros(ops.mx_weight_bytes(Cout, Cin, K, 0) + ops.mx_weight_bytes(Cout, Cin, K, 1),
                         device="cuda", dtype=torch.uint8)
        served = 56 if case == "A2" else 28
        R = lib.avd_mx_stat_rows(served, served, B, K, Cin, Cout, pad)
        assert R > 0
        y = Buf((N, H, W, Cout), sq(N, H, W, Cout), BF)
        stats = Buf((Cout * G * R * 2,), Cout * G * R * 2, torch.float32)
        dx = Buf((N, H, W, Cin), sq(N, H, W, Cin), BF)
        dy = torch.zeros(N * M * M * Cout, device="cuda", dtype=BF)
        rc = [lib.avd_mx_conv_fwd(p(x.t), p(wq), p(wq), None, None, p(y.t), p(stats.t), N, B, Cin, H, W, Cout,
                                  K, pad, st),
              lib.avd_mx_conv_dgrad(p(dy), p(wq), p(wq), p(dx.t), N, Cin, H, W, Cout, K, pad, st)]
        outs = [y, stats, dx]
    torch.cuda.synchronize()
    assert all(r == AVD_ERR_SHAPE for r in rc), rc
    for o in outs:
        o.check(written=False)


@pytest.mark.parametrize("case,H,W", rows_of("avd_cl_conv_fwd", D), ids=["R4-8x64"])
def test_rect_conv3_declines_wide_maps(ops, case, H, W):
    """bf16 3x3, Cin and Cout multiples of 32: conv3.hip's launcher (avd_c3_conv: plan and dispatch
    on the host, AVD_ERR_SHAPE when no instantiation matches) declines W > 62 before any launch,
    forward and input gradient."""
    from avdino._lib import lib
    assert (case, H, W) in rows_of("avd_cl_conv_dgrad", D)
    Cin, Cout, K, pad, N, B = CASES[case]
    p, st = ops.p, ops.stream()
    x = torch.zeros(N, H, W, Cin, device="cuda", dtype=BF)
    dy = torch.zeros(N, H, W, Cout, device="cuda", dtype=BF)
    wk = torch.zeros(max(ops.cl_weight_elems(Cout, Cin, K, 0), ops.cl_weight_elems(Cout, Cin, K, 1)),
                     device="cuda", dtype=BF)
    y = Buf((N, H, W, Cout), sq(N, H, W, Cout), BF)
    dx = Buf((N, H, W, Cin), sq(N, H, W, Cin), BF)
    rc = [lib.avd_cl_conv_fwd(p(x), p(wk), None, p(y.t), None, 1, N, B, Cin, H, W, Cout, K, pad, st),
          lib.avd_cl_conv_dgrad(p(dy), p(wk), p(dx.t), 1, N, Cin, H, W, Cout, K, pad, st)]
    torch.cuda.synchronize()
    assert rc == [AVD_ERR_SHAPE, AVD_ERR_SHAPE], rc
    y.check(written=False), dx.check(written=False)


@pytest.mark.parametrize("which", sorted(ROUTE_LIMITS))
def test_rect_first_layer_route_limits(ops, which):
    """The per-axis rules of the first-layer routes as include/avdino.h states them, at their edges."""
    N, B = 4, 2
    for Cout, K, pad, H, W, verdict in ROUTE_LIMITS[which]:
        if which == "rows":
            got = [ops.cl_c1_recompute_rows(pas, BF, N, B, 1, H, W, Cout, K, pad) for pas in range(5)]
        else:
            got = [ops.cl_apply_wgrad_slabs(BF, N, 1, H, W, Cout, K, pad)]
        if verdict == S:
            assert all(v > 0 for v in got), (Cout, K, H, W, got)
        else:
            assert all(v == 0 for v in got), (Cout, K, H, W, got)
