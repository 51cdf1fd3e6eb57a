"""The case table, data generators and float64 references of the bit-exact conv-block tests
(tests/test_conv_exact_cases_cpu.py checks them without a device, tests/test_gpu_conv_exact.py
runs the kernels against them).

Data.  x, w and dy are small integers, the bias a multiple of 0.5 in [-4, 4]: all exact in bf16
and f32, and every product and partial sum of a conv over them is an integer (or half-integer)
far below 2^24, so f32 accumulation is exact in any order on either MFMA.  The only rounding
left is the final store: a kernel's output must equal bf16_rne(float32(exact)) bit for bit.

  "map" data   integers in [-lim, lim], lim = 3 (7 for Cin = 1: with [-3, 3] a single-channel
               conv cannot leave the range |y| <= 9 K^2 + 4 <= 229 that bf16 stores without
               rounding).  One output channel -- the last, so the one in the ragged MFMA tile
               where there is one -- gets weights of +-lim only and the input a patch of
               lim sign(w) in the last sample, so that y there is lim^2 Cin K^2 (+ bias) and its
               neighbours (partial overlaps of the patch) spread over the binades above 256,
               where bf16 rounds integers: the store's rounding, exact ties included, is
               exercised, which test_conv_exact_cases_cpu.py asserts per case.
  "stats" data integers in {-1, 0, 1}: |y| stays small enough that the stored bf16 value is the
               exact value, so the BatchNorm partial sums (sum y, sum y^2, or about a pivot) are
               exact too and the "stored y" and "exact y" definitions of them coincide.

A case is (N, B, Cin, H, W, Cout, K, pad, kinds, rows):
  kinds  the entry points it is run through, of "f" (avd_cl_conv_fwd), "d" (avd_cl_conv_dgrad),
         "w" (avd_cl_conv_wgrad).  Not every (entry point, type) serves every row: the generic
         forward / input-gradient kernels are instantiated for 8, 16, 32, 64 (3x3: also 128, 256)
         channels of the map they READ, x in the forward and dy in the input gradient, and return
         AVD_ERR_SHAPE before any launch for another count (include/avdino.h); serves() states
         the rule, and the rows it declines are tested as declined.  A row of the first nine
         whose kinds leave out "d" is declined there in both types; "dw" rows are the mirror
         images (forward declined) that give the input gradient its ragged output channels.
  rows   (f32, bf16) avd_cl_stat_rows of the forward: pins the tiling the case was chosen for
         (plan_cl: 4 rows per block and BN group; conv_c1p.hip: 4 B).  "4cu" = conv3.hip's 4 rows
         per compute unit; None = no forward.
"""
import functools

import torch

F64 = torch.float64
SERVED_CH = {3: (8, 16, 32, 64, 128, 256), 5: (8, 16, 32, 64)}   # read-map channels, per K

# ---- generic conv_cl kernels (f32 and bf16; bf16 3x3 with Cin, Cout % 32 == 0 is conv3.hip's)
GENERIC = [
    # ragged Cout in NT = 4; forward tile 16 wide on an 11-wide map
    (6, 3, 8, 9, 11, 40, 3, 1, "fw", (12, 12)),
    # two channel blocks, the second ragged; NS = 4 whole-map packing; odd map
    (4, 4, 16, 7, 7, 72, 3, 1, "fw", (4, 4)),
    # two 32-channel LDS chunks; bf16 forward packs NS = 3 with 7 pixel groups per wave
    (3, 3, 64, 10, 10, 24, 5, 2, "fw", (12, 4)),
    # four LDS chunks; bf16 3x3 stays generic because Cout % 32 != 0
    (2, 2, 128, 9, 7, 40, 3, 1, "fw", (4, 4)),
    # 7 tiles across
    (2, 1, 8, 20, 70, 16, 5, 2, "fdw", (28, 28)),
    # 3 tiles down, the last ragged: 33 = 13 + 13 + 7
    (2, 1, 8, 33, 19, 16, 5, 2, "fdw", (12, 12)),
    # 2x2 tiles with 7 pixel groups per wave
    (2, 2, 16, 40, 44, 32, 3, 1, "fdw", (32, 32)),
    # odd sizes; ragged last row tile
    (2, 1, 16, 23, 37, 40, 5, 2, "fw", (16, 16)),
    # unpadded; forward NS = 2 (10x10 outputs), input gradient NS = 2 in bf16
    (6, 2, 16, 14, 14, 32, 5, 0, "fdw", (4, 4)),
    # the input gradient's ragged output channels (its "Cout" is Cin): NT = 4 with 40 of 64, NS = 2
    (6, 3, 40, 9, 11, 8, 3, 1, "dw", None),
    # ... two channel blocks, the second ragged, NS = 4
    (4, 4, 72, 7, 7, 16, 3, 1, "dw", None),
    # ... 24 of 32 channels from two LDS chunks of dy; weight gradient with Cin 24 padded to 32
    (3, 3, 24, 10, 10, 64, 5, 2, "dw", None),
    # pad 0: 4x4 outputs, NS = 6; Cin 24
    (6, 6, 24, 6, 6, 8, 3, 0, "dw", None),
]

# ---- first layers (Cin = 1): conv_c1_kernel / wgrad_c1_kernel; the last two are conv_c1p.hip's
# pixel-pair route in bf16, at its smallest and widest served maps
CIN1 = [
    (4, 2, 1, 18, 22, 24, 3, 1, "fw", (4, 4)),      # 7 groups per wave, 2 batches, NS = 2
    (2, 1, 1, 37, 23, 24, 5, 2, "fw", (4, 4)),      # 7 groups per wave, 2 batches
    (4, 2, 1, 30, 26, 40, 5, 2, "fw", (4, 4)),      # 7 batches
    (2, 2, 1, 50, 38, 8, 3, 1, "fw", (8, 8)),       # 8 batches
    (2, 2, 1, 64, 48, 16, 3, 1, "fw", (16, 16)),    # 2 tiles of 6 batches
    (2, 1, 1, 16, 16, 8, 5, 2, "fw", (4, 4)),
    (2, 1, 1, 16, 112, 8, 5, 2, "fw", (4, 4)),
]

# ---- conv3.hip (bf16 3x3 pad 1, Cin and Cout multiples of 32): every (BO, GPW, IW8) its plan3
# returns and its dispatch instantiates; the f32 runs of these rows take the generic kernels.
CONV3 = [                                            # BO GPW IW8
    (4, 2, 32, 4, 3, 64, 3, 1, "fdw", (4, "4cu")),       # 64  4  16   NS = 2, odd W
    (2, 1, 32, 3, 5, 96, 3, 1, "fdw", (4, "4cu")),       # 32  4  16   O = 96
    (3, 3, 64, 7, 13, 64, 3, 1, "fdw", (12, "4cu")),     # 64  7  16   NS = 3, two input chunks
    (2, 2, 32, 20, 13, 32, 3, 1, "fdw", (8, "4cu")),     # 32  7  16
    (2, 2, 32, 20, 15, 128, 3, 1, "fdw", (16, "4cu")),   # 64  4  32   tiles of 17 + 3 rows
    (3, 3, 32, 3, 15, 96, 3, 1, "fdw", (4, "4cu")),      # 32  4  32   NS = 3
    (2, 1, 32, 9, 29, 256, 3, 1, "fdw", (8, "4cu")),     # 64  7  32   O = 256
    (3, 3, 32, 5, 19, 32, 3, 1, "fdw", (4, "4cu")),      # 32  7  32   NS = 3
    (2, 1, 32, 9, 47, 64, 3, 1, "fdw", (8, "4cu")),      # 64  4  64   tiles of 5 + 4 rows
    (2, 1, 32, 3, 62, 96, 3, 1, "fdw", (4, "4cu")),      # 32  4  64   W = 62, the limit
    (2, 2, 32, 13, 53, 64, 3, 1, "fdw", (32, "4cu")),    # 64  7  64   tiles of 8 + 5 rows
    (2, 2, 32, 3, 49, 32, 3, 1, "fdw", (8, "4cu")),      # 32  7  64   NS = 2
    # W = 31..46 pads its rows to 48 pixels, a stride conv3.hip does not instantiate: they run
    # on the 64-pixel kernels
    (2, 1, 32, 5, 33, 64, 3, 1, "fdw", (4, "4cu")),      # 64  4  64
    (2, 2, 32, 4, 46, 96, 3, 1, "fdw", (8, "4cu")),      # 32  7  64   NS = 2
    # N = 5: the weight gradient's 8 slabs (grid % 8 == 0) do not divide the 5 samples
    (5, 5, 32, 8, 12, 64, 3, 1, "fdw", (20, "4cu")),
]

# ---- weight-gradient extras (generic wgrad_cl): N = 5, output widths that are no multiple of 8,
# Cin 8 / 24 (the channel block padded to 16 / 32), Cout 24 / 40 / 72
WGRAD = [
    (5, 5, 8, 12, 12, 24, 3, 1, "w", None),
    (5, 1, 24, 9, 13, 40, 5, 2, "w", None),
    (5, 5, 16, 6, 10, 72, 3, 1, "w", None),
]

# ---- the weights-stationary mid layers (conv_ws.hip, wgrad_ws.hip; bf16): test_gpu_cl.py's
# WS_SHAPES at N = 4, B = 2.  rows: of the generic kernel (generic_conv = 1); the persistent
# kernel's rows follow its grid (grid_cap).
WS = [
    (4, 2, 8, 56, 56, 16, 5, 2, "fdw", (56, 56)),
    (4, 2, 16, 28, 28, 32, 5, 2, "fdw", (16, 16)),
    (4, 2, 32, 14, 14, 64, 5, 2, "fdw", (8, 8)),
    (4, 2, 32, 14, 14, 64, 5, 0, "fdw", (4, 4)),
]

TABLE = GENERIC + CIN1 + CONV3 + WGRAD
ALL = TABLE + WS


def cid(case):
    N, B, Cin, H, W, Cout, K, pad = case[:8]
    return f"{N}.{B}x{Cin}x{H}x{W}-{Cout}k{K}p{pad}"


def having(kind, table=None):
    return [c for c in (TABLE if table is None else table) if kind in c[8]]


def serves(case, kind, bf16):
    """Whether entry point `kind` serves the case in f32 (bf16 = False) or bf16, by the rules of
    include/avdino.h: conv3.hip takes the bf16 3x3 pad-1 layers with Cin, Cout % 32 == 0 (the
    written map at most 256 channels, W <= 62); anything else runs on the generic kernels, which
    exist for SERVED_CH channels of the map they read (first layers: forward only)."""
    _, _, Cin, _, W, Cout, K, pad = case[:8]
    if kind == "w":
        return True
    read, written = (Cin, Cout) if kind == "f" else (Cout, Cin)
    if kind == "d" and Cin == 1:
        return False
    if bf16 and K == 3 and pad == 1 and Cin % 32 == 0 and Cout % 32 == 0 and written <= 256:
        return W <= 62
    return read == 1 or read in SERVED_CH[K]


def run_list(kind, table=None):
    """[(case, "f32" | "bf16")] served through entry point `kind`, and the declined ones."""
    rows = [(c, dt) for c in (TABLE if table is None else table) if kind in c[8] for dt in ("f32", "bf16")]
    return ([r for r in rows if serves(r[0], kind, r[1] == "bf16")],
            [r for r in rows if not serves(r[0], kind, r[1] == "bf16")])


def declined_list():
    """[(kind, case, dt)] of the forward / input-gradient calls the table's Cin > 1 rows get
    AVD_ERR_SHAPE from (the rows that exist only for the weight gradient aside)."""
    return [(k, c, dt) for c in TABLE if c[2] > 1 and c[8] != "w" for k in "fd"
            for dt in ("f32", "bf16") if not serves(c, k, dt == "bf16")]


def out_hw(case):
    _, _, _, H, W, _, K, pad = case[:8]
    return H + 2 * pad - K + 1, W + 2 * pad - K + 1


def lim_of(case, kind):
    if kind == "stats":
        return 1
    return 7 if case[2] == 1 else 3


# ------------------------------------------------------------------------------------- data
def _gen(case, salt):
    g = torch.Generator()
    g.manual_seed((hash(case[:8]) + 7919 * salt) % (2 ** 31))
    return g


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64)


@functools.lru_cache(maxsize=None)
def fwd_data(case, kind):
    """(x [N, Cin, H, W], w [Cout, Cin, K, K], bias [Cout]) in float64, NCHW; kind "map", "stats"
    or "gauss" (standard normal x, w / sqrt(Cin K^2), uniform bias)."""
    N, B, Cin, H, W, Cout, K, pad = case[:8]
    g = _gen(case, {"map": 1, "stats": 2, "gauss": 3}[kind])
    if kind == "gauss":
        x = torch.randn(N, Cin, H, W, generator=g, dtype=F64)
        w = torch.randn(Cout, Cin, K, K, generator=g, dtype=F64) / (Cin * K * K) ** 0.5
        return x, w, torch.rand(Cout, generator=g, dtype=F64) - 0.5
    lim = lim_of(case, kind)
    x, w = _ints(g, (N, Cin, H, W), lim), _ints(g, (Cout, Cin, K, K), lim)
    b = torch.randint(-8, 9, (Cout,), generator=g).to(F64) / 2
    if kind == "map":
        # the last channel's weights +-lim, and in the last sample a patch of lim sign(w) under
        # the output pixel nearest the map's centre whose window lies inside the map
        s = torch.where(torch.rand(Cin, K, K, generator=g) < 0.5, -1.0, 1.0).to(F64)
        w[-1] = lim * s
        Ho, Wo = out_hw(case)
        oy, ox = min(max(Ho // 2, pad), H - K + pad), min(max(Wo // 2, pad), W - K + pad)
        x[-1, :, oy - pad:oy - pad + K, ox - pad:ox - pad + K] = lim * s
    return x, w, b


@functools.lru_cache(maxsize=None)
def bwd_data(case, kind):
    """dy [N, Cout, Ho, Wo] float64: integers in [-3, 3], or standard normal."""
    N, Cout = case[0], case[5]
    Ho, Wo = out_hw(case)
    g = _gen(case, {"map": 4, "gauss": 5}[kind])
    if kind == "gauss":
        return torch.randn(N, Cout, Ho, Wo, generator=g, dtype=F64)
    return _ints(g, (N, Cout, Ho, Wo), 3)


# ------------------------------------------------------------------------------- references
# Tap loops in float64 (on whatever device the operands live on): with the integer data every
# intermediate is an exactly represented integer, so the order of the sums is immaterial.
def _taps(K):
    return [(i, j) for i in range(K) for j in range(K)]


def _padded(x, pad):
    return torch.nn.functional.pad(x, (pad, pad, pad, pad))


def conv_fwd64(x, w, b, pad):
    K = w.shape[-1]
    Ho, Wo = x.shape[2] + 2 * pad - K + 1, x.shape[3] + 2 * pad - K + 1
    xp = _padded(x, pad)
    y = torch.zeros(x.shape[0], w.shape[0], Ho, Wo, dtype=F64, device=x.device)
    for i, j in _taps(K):
        y += torch.einsum("nchw,oc->nohw", xp[:, :, i:i + Ho, j:j + Wo], w[:, :, i, j])
    return y + b.view(1, -1, 1, 1)


def conv_dgrad64(dy, w, H, W, pad):
    K = w.shape[-1]
    Ho, Wo = dy.shape[2], dy.shape[3]
    dxp = torch.zeros(dy.shape[0], w.shape[1], H + 2 * pad, W + 2 * pad, dtype=F64, device=dy.device)
    for i, j in _taps(K):
        dxp[:, :, i:i + Ho, j:j + Wo] += torch.einsum("nohw,oc->nchw", dy, w[:, :, i, j])
    return dxp[:, :, pad:pad + H, pad:pad + W].contiguous()


def conv_wgrad64(x, dy, K, pad):
    Ho, Wo = dy.shape[2], dy.shape[3]
    xp = _padded(x, pad)
    dw = torch.zeros(dy.shape[1], x.shape[1], K, K, dtype=F64, device=x.device)
    for i, j in _taps(K):
        dw[:, :, i, j] = torch.einsum("nohw,nchw->oc", dy, xp[:, :, i:i + Ho, j:j + Wo])
    return dw


def rounded(t, rnd):
    """t as the kernels of storage type rnd ("f32", "bf16"; None: as it is) get it, in float64."""
    if rnd is None:
        return t
    return (t.float().bfloat16() if rnd == "bf16" else t.float()).double()


@functools.lru_cache(maxsize=None)
def fwd_ref(case, kind, rnd=None):
    """(y64, scale): the float64 forward and the same sum over absolute values, sum |x||w| + |b|,
    of the operands rounded to rnd (the bias is f32 in both types)."""
    x, w, b = fwd_data(case, kind)
    x, w, b = rounded(x, rnd), rounded(w, rnd), rounded(b, rnd and "f32")
    pad = case[7]
    return conv_fwd64(x, w, b, pad), conv_fwd64(x.abs(), w.abs(), b.abs(), pad)


@functools.lru_cache(maxsize=None)
def dgrad_ref(case, kind, rnd=None):
    w = rounded(fwd_data(case, kind)[1], rnd)
    dy = rounded(bwd_data(case, kind), rnd)
    H, W, pad = case[3], case[4], case[7]
    return conv_dgrad64(dy, w, H, W, pad), conv_dgrad64(dy.abs(), w.abs(), H, W, pad)


@functools.lru_cache(maxsize=None)
def wgrad_ref(case, kind, rnd=None):
    x = rounded(fwd_data(case, kind)[0], rnd)
    dy = rounded(bwd_data(case, kind), rnd)
    K, pad = case[6], case[7]
    return conv_wgrad64(x, dy, K, pad), conv_wgrad64(x.abs(), dy.abs(), K, pad)


def stats_ref(y64, B, pivot=None):
    """[Cout, G, 2] float64: sum (y - pivot) and sum (y - pivot)^2 per channel and BN group."""
    N, C = y64.shape[:2]
    d = y64 if pivot is None else y64 - pivot.view(1, -1, 1, 1)
    d = d.reshape(N // B, B, C, -1)
    return torch.stack([d.sum((1, 3)), (d * d).sum((1, 3))], -1).transpose(0, 1).contiguous()


def bf16_exact(t):
    """True where a float64 value survives f32 -> bf16 (round to nearest even) unchanged."""
    return t.float().bfloat16().double() == t


def bf16_ties(t):
    """True where a float64 value lies exactly halfway between two neighbouring bf16 values."""
    return (t.float().view(torch.int32) & 0xFFFF) == 0x8000


# ---------------------------------------------------------------- BN -> ReLU -> pool block data
POOL_C = (8, 24, 40)
POOL_HW = ((8, 8), (7, 10), (12, 20), (5, 6))
POOL_N, POOL_B = 4, 2


def pool_ref(z):
    """Test-owned 2x2 floor-mode max-pool of z [N, C, H, W] with first-max ties in window order
    (0,0), (0,1), (1,0), (1,1): (pooled [N, C, Hp, Wp], arg [N, C, Hp, Wp] in 0..3)."""
    N, C, H, W = z.shape
    Hp, Wp = H // 2, W // 2
    win = torch.stack([z[:, :, 0:2 * Hp:2, 0:2 * Wp:2], z[:, :, 0:2 * Hp:2, 1:2 * Wp:2],
                       z[:, :, 1:2 * Hp:2, 0:2 * Wp:2], z[:, :, 1:2 * Hp:2, 1:2 * Wp:2]], -1)
    best, arg = win[..., 0].clone(), torch.zeros(N, C, Hp, Wp, dtype=torch.int64, device=z.device)
    for k in (1, 2, 3):
        up = win[..., k] > best
        best = torch.where(up, win[..., k], best)
        arg = torch.where(up, torch.full_like(arg, k), arg)
    return best, arg


def route_ref(dp, arg, H, W):
    """The gradient dp [N, C, Hp, Wp] routed to each window's arg pixel: [N, C, H, W]."""
    N, C, Hp, Wp = dp.shape
    d = torch.zeros(N, C, H, W, dtype=dp.dtype, device=dp.device)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        d[:, :, i:2 * Hp:2, j:2 * Wp:2] = torch.where(arg == k, dp, torch.zeros_like(dp))
    return d


@functools.lru_cache(maxsize=None)
def block_data(C, H, W, N=POOL_N, B=POOL_B, seed=0):
    """Exact operands of the BN -> ReLU -> pool block and its backward, float64:
      y [N, C, H, W] integers in [-6, 6] with planted windows: exact ties (pixel pairs, and all
        four equal) and windows <= 0 after the affine whatever the sign of the scale (y = 0 with
        a shift <= 0 in half of the channels; elsewhere y = -8 sign(scale));
      scale [G, C] = +-2^k, k in -2..1; shift [G, C] multiples of 0.25 in [-2, 2];
      coef [G, C, 3] = (k1, kx, k0): k1 = +-2^k (k in -1..1), kx = +-2^-k (k in 1..5) or 0, k0 a
        quarter-integer in [-1, 1];
      mean [G, C] integers in [-2, 2]; invstd [G, C] = 2^k, k in -2..1;
      gout [N, C, Hp, Wp] integers in [-12, 12] with zeros planted (|dy| reaches 8 and more,
        where bf16 no longer holds its multiples of 1/32: the store of dy rounds)."""
    g = torch.Generator()
    g.manual_seed(1000 * C + 10 * H + W + 77 * seed)
    G, Hp, Wp = N // B, H // 2, W // 2

    def ri(lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=g).to(F64)

    def sign(*s):
        return torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0).to(F64)

    y = ri(-6, 6, N, C, H, W)
    scale = sign(G, C) * 2.0 ** ri(-2, 1, G, C)
    shift = ri(-8, 8, G, C) / 4
    shift[:, ::2] = 0.0 - shift[:, ::2].abs()               # every other channel: shift <= 0 (no -0)
    p = [y[:, :, i:2 * Hp:2, j:2 * Wp:2] for i, j in ((0, 0), (0, 1), (1, 0), (1, 1))]

    def mask(q):
        return torch.rand(N, C, Hp, Wp, generator=g) < q
    m = mask(0.2)
    p[1][m] = p[0][m]
    m = mask(0.1)
    p[3][m] = p[2][m]
    m = mask(0.1)
    p[2][m] = p[0][m]
    m = mask(0.05)
    for q in p[1:]:
        q[m] = p[0][m]
    dead = mask(0.15)
    sg = torch.sign(scale).view(G, 1, C, 1, 1).expand(G, B, C, Hp, Wp).reshape(N, C, Hp, Wp)
    neg = torch.where((torch.arange(C) % 2 == 0).view(1, C, 1, 1), torch.zeros_like(sg), -8.0 * sg)
    for q in p:
        q[dead] = neg[dead]
    k1 = sign(G, C) * 2.0 ** ri(-1, 1, G, C)
    kx = sign(G, C) * 2.0 ** -ri(1, 5, G, C)
    kx[:, 1::5] = 0.0
    k0 = ri(-4, 4, G, C) / 4
    coef = torch.stack([k1, kx, k0], -1).contiguous()
    mean = ri(-2, 2, G, C)
    invstd = 2.0 ** ri(-2, 1, G, C)
    gout = ri(-12, 12, N, C, Hp, Wp)
    gout[mask(0.2)] = 0.0
    return y, scale, shift, coef, mean, invstd, gout


def per_sample(v, N, B):
    """[G, C] -> [N, C, 1, 1]: the coefficient of every sample's group."""
    G, C = v.shape
    return v.view(G, 1, C).expand(G, B, C).reshape(N, C, 1, 1)


def block_ref(y, scale, shift, coef, mean, invstd, gp, B, round_dy=False):
    """float64 reference of the block over NCHW operands; gp = the gradient of the POOLED MAP
    [N, C, Hp, Wp] (mode 1: gout / (Hp Wp) broadcast; mode 2: gout reshaped).  Returns
      pooled [N, C, Hp, Wp], nib [N, C, Hp, Wp] (the routing code: 1 + arg where pooled > 0, else
      0), dz [N, C, H, W], dy [N, C, H, W] = k1 dz + kx y + k0 (bf16-rounded if round_dy), and
      sums [C, G, 2] = (sum dz, sum dz (y - mean) invstd) per channel and group."""
    N, C, H, W = y.shape
    z = y * per_sample(scale, N, B) + per_sample(shift, N, B)
    z = torch.where(z > 0, z, torch.zeros_like(z))          # max(z, +0): no -0 leaves the ReLU
    pooled, arg = pool_ref(z)
    nib = torch.where(pooled > 0, arg + 1, torch.zeros_like(arg))
    dz = route_ref(torch.where(pooled > 0, gp, torch.zeros_like(gp)), arg, H, W)
    k1, kx, k0 = (per_sample(coef[..., i].contiguous(), N, B) for i in range(3))
    dy = k1 * dz + kx * y + k0
    if round_dy:
        dy = dy.float().bfloat16().double()
    xh = (y - per_sample(mean, N, B)) * per_sample(invstd, N, B)
    G = N // B
    s1 = dz.reshape(G, B, C, -1).sum((1, 3))
    s2 = (dz * xh).reshape(G, B, C, -1).sum((1, 3))
    a2 = (dz * xh).abs().reshape(G, B, C, -1).sum((1, 3))
    return pooled, nib, dz, dy, torch.stack([s1, s2], -1).transpose(0, 1).contiguous(), a2


def pivot_of(case):
    """An integer statistics pivot [Cout] in [-2, 2] (float64) for avd_cl_conv_fwd_pv."""
    return torch.randint(-2, 3, (case[5],), generator=_gen(case, 6)).to(F64)


# ------------------------------------------------------------------- fused backward launches
# (N, B, Cin, H, W, Cout, K, pad): avd_cl_layer_bwd[_codes]'s two served shapes, and the first
# layers of avd_cl_bn_bwd_apply_wgrad (conv_c1p.hip: Cout 8, 5x5; c1w3.hip: Cout 32, 3x3)
LAYER_BWD = [(4, 2, 8, 56, 56, 16, 5, 2), (4, 2, 16, 28, 28, 32, 5, 2)]
APPLY_WGRAD = [(4, 2, 1, 16, 16, 8, 5, 2), (4, 2, 1, 8, 20, 32, 3, 1)]


@functools.lru_cache(maxsize=None)
def fused_ref(case):
    """Operands and float64 reference of a fused backward launch: the block data of block_data
    for y [N, Cout, H, W], gout, scale, shift and coef, integer x [N, Cin, H, W] and w in
    [-3, 3]; dy by the rule of csrc/bnapply.h rounded to bf16, then the exact conv gradients of
    that dy.  Returns a dict; "unit" is the common unit of every dy (a power of two), so that
    sum |dy||w| / unit and sum |x||dy| / unit below 2^24 make every f32 partial sum exact."""
    N, B, Cin, H, W, Cout, K, pad = case
    y, scale, shift, coef, mean, invstd, gout = block_data(Cout, H, W, N, B, seed=1)
    g = _gen(case + ("", None), 9)
    x, w = _ints(g, (N, Cin, H, W), 3), _ints(g, (Cout, Cin, K, K), 3)
    _pooled, nib, _dz, dy, _s, _a = block_ref(y, scale, shift, coef, mean, invstd, gout, B, round_dy=True)
    return dict(y=y, scale=scale, shift=shift, coef=coef, gout=gout, x=x, w=w, dy=dy, nib=nib, unit=2.0 ** -5,
                dx=conv_dgrad64(dy, w, H, W, pad), dx_abs=conv_dgrad64(dy.abs(), w.abs(), H, W, pad),
                dw=conv_wgrad64(x, dy, K, pad), dw_abs=conv_wgrad64(x.abs(), dy.abs(), K, pad))
