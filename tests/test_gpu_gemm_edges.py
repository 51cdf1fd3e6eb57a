"""Edge-shape, bit-exact and float64 parity of the dense GEMM family (csrc/gemm.hip): avd_gemm,
avd_linear_bwd and the encoder Linear over NHWC features (avd_linear_*_hwc).

The calls go to the library directly, so the test owns the split-K workspace.  Every case

  * reads operands whose rows are separated by NaN (a leading-dimension gap) and followed by a
    NaN tail: a padded read, even one multiplied by a zeroed LDS lane, poisons the sum;
  * writes into outputs pre-filled with NaN where beta == 0 (C must not be read) and with
    random data otherwise, whose leading-dimension gaps and tail hold a sentinel bit pattern
    that must come back bit for bit;
  * gets a NaN-filled workspace followed by a sentinel tail after exactly *_ws_elems floats;
  * runs on two kinds of data.  Integer data (A, B in [-3, 3]; bias and the old C in [-8, 8];
    alpha, beta halves): every product and partial sum is exact in f32 (and the operands in
    bf16) in any order, below 2^19 at the largest K, so the result must equal the float64
    reference bit for bit in all modes, with or without split-K -- a wrong index, a dropped or
    doubled k, an overlapping split, a wrong column map or beta / bias element cannot hide
    behind a tolerance.  Gaussian data (rounded to bf16 on the host for the bf16 mode): each
    element within the any-order dot-product bound
        |c - c64| <= (K + S + 4) u (|alpha| sum_k |a||b| + |bias| + |beta||c_old|),  u = 2^-24,
    S the split count; a bf16 output adds half a bf16 ulp of the reference value.  The largest
    |err| / (u scale) of each test is printed next to K + S + 4 (-s).  For the f32 modes the
    bound is derived; the bf16 MFMA's internal accumulation is not documented, and was measured
    on an MI355X to stay inside the same bound on every case (at most 2.8 where the f32 modes
    reach 6.6, against bounds from 41 up), so mode 2 is held to it too.

The tile and split count of each case are literals of tests/gemm_cases.py, asserted here through
*_ws_elems and pinned without a device by test_gemm_args_cpu.py.
"""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import gemm_cases as GC  # noqa: E402

U = 2.0 ** -24
GUARD = 64
SENT32 = 0x7FC5A5A5            # f32 sentinel bits: a NaN with a payload
SENT16 = 0x7FC5                # bf16 sentinel bits
NAN = float("nan")
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from avdino import ops as _ops
    return _ops


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g, device=DEV).float()


def gauss(g, shape, bf16=False):
    t = torch.randn(shape, generator=g, device=DEV)
    return t.bfloat16().float() if bf16 else t


def bf16_round(t):
    return t.bfloat16().float()


# --------------------------------------------------------------------------------- buffers
class In2d:
    """A read-only [r, c] matrix at element offset ``lead`` of a NaN-filled allocation, rows
    ``c + pad`` apart, followed by a NaN tail of 40 more rows (a read past the last row, of a
    whole row chunk say, stays inside the allocation and poisons the result)."""

    def __init__(self, vals, pad=0, lead=0):
        r, c = vals.shape
        self.ld = c + pad
        self.full = torch.full((lead + (r + 40) * self.ld + GUARD,), NAN, dtype=vals.dtype, device=DEV)
        self.full[lead:lead + r * self.ld].view(r, self.ld)[:, :c] = vals
        self.ptr = self.full.data_ptr() + lead * vals.element_size()


class Out2d:
    """An output [r, c] at element offset ``lead`` of an allocation, rows ``c + pad`` apart,
    pre-filled with ``init`` (NaN without one); everything around it is a sentinel bit pattern."""

    def __init__(self, r, c, pad=0, lead=0, init=None, dtype=torch.float32):
        self.r, self.c, self.ld, self.lead = r, c, c + pad, lead
        n = lead + r * self.ld + GUARD
        idt, sent = (torch.int32, SENT32) if dtype == torch.float32 else (torch.int16, SENT16)
        self.full = torch.full((n,), sent, dtype=idt, device=DEV).view(dtype)
        self.sent = self.full.view(idt).clone()
        self.idt = idt
        self.view()[:] = NAN if init is None else init
        self.ptr = self.full.data_ptr() + lead * self.full.element_size()

    def view(self, full=None):
        full = self.full if full is None else full
        return full[self.lead:self.lead + self.r * self.ld].view(self.r, self.ld)[:, :self.c]

    def take(self):
        """The result, after checking that nothing around it was written."""
        got = self.full.view(self.idt).clone()
        out = self.view().clone()
        self.view(got.view(self.full.dtype)).zero_()
        ref = self.sent.clone()
        self.view(ref.view(self.full.dtype)).zero_()
        assert torch.equal(got, ref), "a write outside the output (gap, lead or tail)"
        return out


class Ws:
    """A NaN-filled workspace of ``need`` floats followed by a sentinel tail."""

    def __init__(self, need):
        self.need = need
        self.full = torch.full((need + GUARD,), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)
        self.full[:need] = NAN
        self.ptr = self.full.data_ptr()

    def check(self):
        tail = self.full[self.need:].view(torch.int32)
        assert bool((tail == SENT32).all()), "a write past *_ws_elems floats of the workspace"


def ws_args(need, how):
    """(Ws or None, pointer, ws_elems) of the three workspace choices."""
    if how == "null" or need == 0:
        return None, None, 0
    w = Ws(need)
    return w, w.ptr, need - 1 if how == "short" else need


# ------------------------------------------------------------------------------ references
def prod64(A, B):
    """(A B, |A| |B|) in float64 on the device."""
    A, B = A.double(), B.double()
    return A @ B, A.abs() @ B.abs()


def half_ulp_bf16(ref):
    _, ex = torch.frexp(ref)                       # |ref| = m 2^ex, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), ex - 9))


def ratio(got, ref, scale, extra=None):
    """max |got - ref| / (u scale), the half-ulp allowance of a bf16 output taken off first."""
    err = (got.double() - ref).abs()
    assert not bool(torch.isnan(err).any()), "NaN in the result (an element not written, or a padded read)"
    if extra is not None:
        err = (err - extra).clamp_min(0)
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "an error where the bound is zero"
    return float((err / (U * scale.masked_fill(zero, 1.0))).max()) if err.numel() else 0.0


class Report:
    """The largest error ratio of a test and the bound it was held to, printed once."""

    def __init__(self, capsys, what):
        self.capsys, self.what, self.worst, self.bound = capsys, what, 0.0, 0

    def add(self, tag, r, bound):
        if r >= self.worst:
            self.worst, self.bound = r, bound
        assert r <= bound, f"{self.what} {tag}: |err| / (u scale) = {r:.2f} > {bound}"

    def done(self):
        with self.capsys.disabled():
            print(f"\n[gemm-edges] {self.what}: max |err|/(u scale) {self.worst:.2f}, bound {self.bound}", end="")


# ------------------------------------------------------------------------------- avd_gemm
# operand storage: (contiguous along k?, leading-dimension pad, base offset in floats)
def store_a(A, kfast, pad=0, lead=0):
    """A [M, K] -> (In2d, sam, sak)."""
    b = In2d(A if kfast else A.t().contiguous(), pad, lead)
    return (b, b.ld, 1) if kfast else (b, 1, b.ld)


def store_b(B, kfast, pad=0, lead=0):
    """B [K, N] -> (In2d, sbk, sbn); k-contiguous storage is B^T [N, K]."""
    b = In2d(B.t().contiguous() if kfast else B, pad, lead)
    return (b, 1, b.ld) if kfast else (b, b.ld, 1)


def call_gemm(ops, M, N, K, a, b, mode, bias=None, alpha=1.0, beta=0.0, cold=None, cpad=0,
              need=0, how="full"):
    """One avd_gemm over stored operands a, b (store_a / store_b) -> C [M, N]."""
    (ab, sam, sak), (bb, sbk, sbn) = a, b
    assert (beta == 0.0) == (cold is None)
    out = Out2d(M, N, pad=cpad, init=cold)
    w, wp, we = ws_args(need if mode else 0, how)
    ops.call("avd_gemm", M, N, K, ab.ptr, sam, sak, bb.ptr, sbk, sbn, out.ptr, out.ld,
             None if bias is None else bias.data_ptr(), alpha, beta, mode, wp, we, ops.stream())
    res = out.take()
    if w is not None:
        w.check()
    return res


class GemmData:
    """Operands and float64 products of one (case, kind of data), made once per case."""

    def __init__(self, M, N, K, kind, seed):
        g = gen(seed)
        self.kind = kind
        if kind == "int":
            self.A, self.B = ints(g, (M, K), 3), ints(g, (K, N), 3)
            self.bias, self.cold = ints(g, (N,), 8), ints(g, (M, N), 8)
        else:
            bf = kind == "gauss_bf16"
            self.A, self.B = gauss(g, (M, K), bf), gauss(g, (K, N), bf)
            self.bias, self.cold = gauss(g, (N,)), gauss(g, (M, N))
        self.P, self.Pabs = prod64(self.A, self.B)

    def ref(self, alpha, beta, bias):
        r, s = alpha * self.P, abs(alpha) * self.Pabs
        if bias:
            r, s = r + self.bias.double(), s + self.bias.double().abs()
        if beta != 0.0:
            r, s = r + beta * self.cold.double(), s + abs(beta) * self.cold.double().abs()
        return r, s


_DATA = {}


def gemm_data(case, kind):
    """Cached for the case at hand only (the parameters run case by case)."""
    M, N, K = case[:3]
    if _DATA.get("case") != (M, N, K):
        _DATA.clear()
        _DATA["case"] = (M, N, K)
    if kind not in _DATA:
        _DATA[kind] = GemmData(M, N, K, kind, 1000003 * M + 1009 * N + K + len(kind))
    return _DATA[kind]


def kinds_of(mode):
    return ("int", "gauss_bf16" if mode == 2 else "gauss")


def check_gemm(rep, tag, got, d, K, S, alpha, beta, bias):
    ref, scale = d.ref(alpha, beta, bias)
    if d.kind == "int":
        assert torch.equal(got, ref.float()), f"{tag}: integer data is not bit-exact"
    else:
        rep.add(tag, ratio(got, ref, scale), K + S + 4)


GEMM_PARAMS = [pytest.param(c, m, id=f"{GC.gemm_id(c)}-m{m}") for c in GC.GEMM_CASES for m in c[6]]


@pytest.mark.parametrize("case,mode", GEMM_PARAMS)
def test_gemm_cases(ops, capsys, case, mode):
    """Each case: a plain call (beta = 0 over a NaN C) and one with bias, alpha, beta and
    ldc = N + 5 over a random old C; split cases also the workspace contract: no workspace and
    one float too few take the single pass and agree bit for bit, a NaN-poisoned full workspace
    changes nothing, nothing is written past it, a second call after ops.lds_poison() repeats
    every bit."""
    M, N, K, tile, S, _, _ = case
    need = GC.gemm_need(case)
    assert ops.lib.avd_gemm_ws_elems(M, N, K, mode) == (need if mode else 0)
    assert (need // (M * N) if need else 1) == S
    rep = Report(capsys, f"gemm {GC.gemm_id(case)} m{mode}")
    # 70x130x45: both operands k-contiguous with rows 48 apart -- aligned rows, K % 4 != 0, so the
    # whole-vector loads are not allowed and would read the NaN gap
    odd45 = (M, N, K) == (70, 130, 45)
    for kind in kinds_of(mode):
        d = gemm_data(case, kind)
        a, b = store_a(d.A, True, 3 if odd45 else 4), store_b(d.B, odd45, 3 if odd45 else 4)
        S_eff = S if mode else 1
        plain = call_gemm(ops, M, N, K, a, b, mode, need=need)
        check_gemm(rep, f"{kind} plain", plain, d, K, S_eff, 1.0, 0.0, False)
        ep = dict(bias=d.bias, alpha=-2.0, beta=-0.5, cold=d.cold, cpad=5, need=need)
        full = call_gemm(ops, M, N, K, a, b, mode, **ep)
        check_gemm(rep, f"{kind} epilogue", full, d, K, S_eff, -2.0, -0.5, True)
        ops.lds_poison()
        assert same_bits(full, call_gemm(ops, M, N, K, a, b, mode, **ep)), "a second call differs"
        if S > 1 and mode:
            null = call_gemm(ops, M, N, K, a, b, mode, **dict(ep, how="null"))
            short = call_gemm(ops, M, N, K, a, b, mode, **dict(ep, how="short"))
            check_gemm(rep, f"{kind} no workspace", null, d, K, 1, -2.0, -0.5, True)
            assert same_bits(null, short), "ws = NULL and ws_elems = need - 1 differ"
            if kind == "int":
                assert same_bits(null, full)
    rep.done()


# operand layouts of the matrix: name -> (A: k-contiguous, pad, lead), (B: the same)
LAYOUTS = {
    "KK-pad4": ((True, 4, 0), (True, 4, 0)),
    "KR-pad4": ((True, 4, 0), (False, 4, 0)),
    "RR-pad4": ((False, 4, 0), (False, 4, 0)),
    "RK-pad4": ((False, 4, 0), (True, 4, 0)),
    "KK-dense": ((True, 0, 0), (True, 0, 0)),
    "KK-pad2": ((True, 2, 0), (True, 2, 0)),            # K = 1030: rows 1032 apart, K % 4 != 0
    "K+stride1": ((True, 4, 0), (True, 1, 0)),          # vector A, scalar B: both scalar
    "offset1+R": ((True, 4, 1), (False, 4, 0)),         # unaligned A, vector B: both scalar
    "R+offset1": ((False, 4, 0), (False, 4, 1)),
    "stride1-both": ((False, 1, 0), (False, 1, 1)),
    "aligned-lead4": ((True, 4, 4), (False, 4, 4)),
}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(132, 68, 100), (256, 200, 1030)], ids=["132x68x100", "256x200x1030-split4"])
def test_gemm_layout_matrix(ops, capsys, shape, mode):
    """The same logical problem from every operand storage: (K,K), (K,R), (R,R), (R,K) vector
    pairs, a vector operand beside a scalar one in both orders (the pair falls to the scalar
    staging), a base pointer one float off, row strides of extent + 1 and padded extent + 4
    with NaN in the padding.  Each within the bound; bit-identical across layouts on integers."""
    case = GC.find_gemm(*shape)
    M, N, K, _, S = case[:5]
    need = GC.gemm_need(case)
    rep = Report(capsys, f"layouts {GC.gemm_id(case)} m{mode}")
    for kind in kinds_of(mode):
        d = gemm_data(case, kind)
        first = None
        for name, (sa, sb) in LAYOUTS.items():
            got = call_gemm(ops, M, N, K, store_a(d.A, *sa), store_b(d.B, *sb), mode, bias=d.bias,
                            alpha=0.5, beta=1.0, cold=d.cold, cpad=5, need=need)
            check_gemm(rep, f"{kind} {name}", got, d, K, S if mode else 1, 0.5, 1.0, True)
            if kind == "int":
                first = got if first is None else first
                assert same_bits(got, first), f"{name} differs from {next(iter(LAYOUTS))}"
    rep.done()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(132, 68, 100), (256, 200, 1030)], ids=["132x68x100", "256x200x1030-split4"])
def test_gemm_epilogue(ops, capsys, shape, mode):
    """bias alone, alpha alone, and both with beta (ldc = N and N + 5), split and unsplit."""
    case = GC.find_gemm(*shape)
    M, N, K, _, S = case[:5]
    need = GC.gemm_need(case)
    rep = Report(capsys, f"epilogue {GC.gemm_id(case)} m{mode}")
    for kind in kinds_of(mode):
        d = gemm_data(case, kind)
        a, b = store_a(d.A, False, 4), store_b(d.B, True, 4)
        for alpha, beta, bias, cpad in [(1.0, 0.0, True, 0), (0.5, 0.0, False, 5), (-2.0, 0.0, False, 0),
                                        (1.0, 1.0, False, 5), (0.5, -0.5, True, 0), (-2.0, 1.0, True, 5)]:
            got = call_gemm(ops, M, N, K, a, b, mode, bias=d.bias if bias else None, alpha=alpha,
                            beta=beta, cold=d.cold if beta else None, cpad=cpad, need=need)
            check_gemm(rep, f"{kind} alpha {alpha} beta {beta} bias {bias}", got, d, K,
                       S if mode else 1, alpha, beta, bias)
    rep.done()


# ------------------------------------------------------------------------- avd_linear_bwd
class BwdData:
    def __init__(self, rows, O, In, kind, seed):
        g = gen(seed)
        self.kind = kind
        if kind == "int":
            self.dout, self.x, self.W = ints(g, (rows, O), 3), ints(g, (rows, In), 3), ints(g, (O, In), 3)
        else:
            bf = kind == "gauss_bf16"
            self.dout, self.x, self.W = gauss(g, (rows, O), bf), gauss(g, (rows, In), bf), gauss(g, (O, In), bf)
        self.dW, self.dWabs = prod64(self.dout.t(), self.x)
        self.dX, self.dXabs = prod64(self.dout, self.W)
        self.db, self.dbabs = self.dout.double().sum(0), self.dout.double().abs().sum(0)


def call_bwd(ops, rows, O, In, dout, x, W, mode, which, db, need, how="full"):
    """One avd_linear_bwd -> (dW, dX, db) (None for what was not asked for); dX is a column
    slice, 3 floats into rows In + 7 wide."""
    dW = Out2d(O, In) if which & 1 else None
    dX = Out2d(rows, In, pad=7, lead=3) if which & 2 else None
    dbo = Out2d(1, O) if db else None
    w, wp, we = ws_args(need, how)
    ops.call("avd_linear_bwd", rows, O, In, dout.ptr, dout.ld, x.ptr if which & 1 else None, x.ld,
             W.ptr if which & 2 else None, dW.ptr if dW else None, dX.ptr if dX else None,
             dX.ld if dX else In, dbo.ptr if dbo else None, mode, which, wp, we, ops.stream())
    res = tuple(o.take() if o else None for o in (dW, dX, dbo))
    if w is not None:
        w.check()
    return res


def gemm_pair(ops, rows, O, In, dout, x, W, mode, how):
    """The two avd_gemm calls avd_linear_bwd stands for, each with its own workspace."""
    n1 = ops.lib.avd_gemm_ws_elems(O, In, rows, mode)
    n2 = ops.lib.avd_gemm_ws_elems(rows, In, O, mode)
    dW, dX = Out2d(O, In), Out2d(rows, In, pad=7, lead=3)
    w1, p1, e1 = ws_args(n1, how)
    ops.call("avd_gemm", O, In, rows, dout.ptr, 1, dout.ld, x.ptr, x.ld, 1, dW.ptr, In, None, 1.0, 0.0,
             mode, p1, e1, ops.stream())
    w2, p2, e2 = ws_args(n2, how)
    ops.call("avd_gemm", rows, In, O, dout.ptr, dout.ld, 1, W.ptr, In, 1, dX.ptr, dX.ld, None, 1.0, 0.0,
             mode, p2, e2, ops.stream())
    for w in (w1, w2):
        if w is not None:
            w.check()
    return dW.take(), dX.take()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", GC.LINEAR_BWD_CASES, ids=GC.linear_bwd_id)
def test_linear_bwd_cases(ops, capsys, case, mode):
    """which = 3 against float64; which = 1 and which = 2 (the launches the step makes on two
    streams) bit-identical to it; all bit-identical to the two avd_gemm calls with the same
    workspace choice (full, or none: single passes, db = NULL).  dout has a NaN gap
    (dout_ld = O + 4 keeps the paired launch's vector layouts; O = 130 gets 136: rows a multiple
    of 4 apart whose extent is not)."""
    rows, O, In, xpad, _, s1, s2, need = case
    assert ops.lib.avd_linear_bwd_ws_elems(rows, O, In, mode) == need
    rep = Report(capsys, f"linear_bwd {GC.linear_bwd_id(case)} m{mode}")
    for kind in kinds_of(mode):
        d = BwdData(rows, O, In, kind, 7919 * rows + 31 * O + In)
        dout, x, W = In2d(d.dout, 4 + -O % 4), In2d(d.x, xpad if xpad else 4), In2d(d.W)
        dW3, dX3, db3 = call_bwd(ops, rows, O, In, dout, x, W, mode, 3, True, need)
        dW1, _, db1 = call_bwd(ops, rows, O, In, dout, x, W, mode, 1, True, need)
        _, dX2, _ = call_bwd(ops, rows, O, In, dout, x, W, mode, 2, False, need)
        dWg, dXg = gemm_pair(ops, rows, O, In, dout, x, W, mode, "full")
        assert same_bits(dW3, dW1) and same_bits(db3, db1), "which = 1 differs from which = 3"
        assert same_bits(dX3, dX2), "which = 2 differs from which = 3"
        assert same_bits(dW3, dWg) and same_bits(dX3, dXg), "differs from the two avd_gemm calls"
        ops.lds_poison()
        again = call_bwd(ops, rows, O, In, dout, x, W, mode, 3, True, need)
        assert all(same_bits(p, q) for p, q in zip((dW3, dX3, db3), again)), "a second call differs"
        dWn, dXn, _ = call_bwd(ops, rows, O, In, dout, x, W, mode, 3, False, need, how="null")
        dWgn, dXgn = gemm_pair(ops, rows, O, In, dout, x, W, mode, "null")
        assert same_bits(dWn, dWgn) and same_bits(dXn, dXgn), "no workspace: differs from avd_gemm"
        if kind == "int":
            for got, ref in [(dW3, d.dW), (dWn, d.dW), (dX3, d.dX), (dXn, d.dX), (db3[0], d.db)]:
                assert torch.equal(got, ref.float()), "integer data is not bit-exact"
        else:
            rep.add(f"{kind} dW", ratio(dW3, d.dW, d.dWabs), rows + s1 + 4)
            rep.add(f"{kind} dW single pass", ratio(dWn, d.dW, d.dWabs), rows + 1 + 4)
            rep.add(f"{kind} dX", ratio(dX3, d.dX, d.dXabs), O + s2 + 4)
            rep.add(f"{kind} dX single pass", ratio(dXn, d.dX, d.dXabs), O + 1 + 4)
            rep.add(f"{kind} db", ratio(db3[0], d.db, d.dbabs), rows + 4)
    rep.done()


@pytest.mark.parametrize("rows,O", GC.DB_CASES)
def test_linear_bwd_bias_gradient_edges(ops, capsys, rows, O):
    """db over one-row chunks (rows <= 128), ragged last chunks and ragged 256-column strips,
    dout_ld > O with NaN in the gap; which = 1 and 3 agree."""
    In, mode = 8, 1
    need = ops.lib.avd_linear_bwd_ws_elems(rows, O, In, mode)
    rep = Report(capsys, f"db {rows}x{O}")
    for kind in ("int", "gauss"):
        d = BwdData(rows, O, In, kind, 104729 * rows + O)
        dout, x, W = In2d(d.dout, 4 if O % 4 == 0 else 3), In2d(d.x), In2d(d.W)
        dW3, dX3, db3 = call_bwd(ops, rows, O, In, dout, x, W, mode, 3, True, need)
        dW1, _, db1 = call_bwd(ops, rows, O, In, dout, x, W, mode, 1, True, need)
        assert same_bits(db3, db1) and same_bits(dW3, dW1)
        if kind == "int":
            assert torch.equal(db3[0], d.db.float()) and torch.equal(dW3, d.dW.float())
            assert torch.equal(dX3, d.dX.float())
        else:
            rep.add("db", ratio(db3[0], d.db, d.dbabs), rows + 4)
    rep.done()


# ------------------------------------------------------------------------------------ _hwc
def to_chw(t, C, HW):
    """[..., (hw, c)] -> [..., (c, hw)]."""
    return t.reshape(*t.shape[:-1], HW, C).transpose(-1, -2).reshape(t.shape)


class HwcData:
    def __init__(self, rows, O, C, HW, kind, seed):
        g = gen(seed)
        In = C * HW
        self.kind = kind
        if kind == "int":
            self.feat, self.W = ints(g, (rows, In), 3), ints(g, (O, In), 3)           # W in (c, h, w)
            self.bias, self.dout = ints(g, (O,), 8), ints(g, (rows, O), 3)
        else:
            self.feat, self.W = gauss(g, (rows, In), True), gauss(g, (O, In))
            self.bias, self.dout = gauss(g, (O,)), gauss(g, (rows, O))                 # dout: raw f32
        self.Wp = to_chw(bf16_round(self.W), HW, C)                                    # (c,hw) -> (hw,c)
        dr = bf16_round(self.dout)                       # the staging rounds dout to bf16 (RNE)
        self.out, self.outabs = prod64(self.feat, self.Wp.t())
        self.out, self.outabs = self.out + self.bias.double(), self.outabs + self.bias.double().abs()
        dW, dWabs = prod64(dr.t(), self.feat)
        self.dW, self.dWabs = to_chw(dW, C, HW), to_chw(dWabs, C, HW)
        self.dX, self.dXabs = prod64(dr, self.Wp)
        self.db, self.dbabs = self.dout.double().sum(0), self.dout.double().abs().sum(0)


def hwc_weight(ops, W, C, HW):
    O, In = W.shape
    Wp = Out2d(1, O * In, dtype=torch.bfloat16)
    P, I = ctypes.c_void_p, ctypes.c_int
    ops.call("avd_linear_weight_hwc", 1, (P * 1)(W.data_ptr()), (P * 1)(Wp.ptr), (I * 1)(O), (I * 1)(C),
             (I * 1)(HW), ops.stream())
    return Wp.take().view(O, In)


def call_hwc_bwd(ops, rows, O, C, HW, dout, feat, Wp, which, need, dx_lead=0):
    In = C * HW
    dW = Out2d(O, In) if which & 1 else None
    db = Out2d(1, O) if which & 1 else None
    dX = Out2d(rows, In, lead=dx_lead, dtype=torch.bfloat16) if which & 2 else None
    w = Ws(need)
    ops.call("avd_linear_bwd_hwc", rows, O, C, HW, dout.ptr, dout.ld, feat.ptr if which & 1 else None,
             Wp.ptr if which & 2 else None, dW.ptr if dW else None, db.ptr if db else None,
             dX.ptr if dX else None, which, w.ptr, need, ops.stream())
    res = tuple(o.take() if o else None for o in (dW, db, dX))
    w.check()
    return res


@pytest.mark.parametrize("case", GC.HWC_CASES, ids=GC.hwc_id)
def test_hwc_cases(ops, capsys, case):
    """The encoder Linear over NHWC bf16 features: the weight permutation, the forward (with and
    without the split-K workspace), dW in the reference's (c, h, w) order through the column map,
    db, and the bf16 dX = RNE of the exact value on integers; which = 1 / 2 against 3; a dX that
    starts 8 bytes into its allocation (the scalar tail of the bf16 tile store) against the
    aligned one.  The Gaussian dout is not pre-rounded: the staging's rounding is RNE."""
    rows, O, C, HW, sf, s1, s2, need = case
    In = C * HW
    assert ops.lib.avd_linear_hwc_ws_elems(rows, O, In) == need
    rep = Report(capsys, f"hwc {GC.hwc_id(case)}")
    for kind in ("int", "gauss"):
        d = HwcData(rows, O, C, HW, kind, 15485863 * rows + 7 * O + In)
        Wp_t = hwc_weight(ops, d.W, C, HW)
        assert same_bits(Wp_t, d.Wp.bfloat16()), "avd_linear_weight_hwc"
        feat, Wp = In2d(d.feat.bfloat16()), In2d(Wp_t)
        outs = []
        for how in ("full", "null"):
            out = Out2d(rows, O, pad=5)
            w, wp, we = ws_args(need, how)
            ops.call("avd_linear_fwd_hwc", rows, O, C, HW, feat.ptr, Wp.ptr, d.bias.data_ptr(), out.ptr,
                     out.ld, wp, we, ops.stream())
            outs.append(out.take())
            if w is not None:
                w.check()
        dout = In2d(d.dout, 4)
        dW3, db3, dX3 = call_hwc_bwd(ops, rows, O, C, HW, dout, feat, Wp, 3, need)
        dW1, db1, _ = call_hwc_bwd(ops, rows, O, C, HW, dout, feat, Wp, 1, need)
        _, _, dX2 = call_hwc_bwd(ops, rows, O, C, HW, dout, feat, Wp, 2, need)
        _, _, dXu = call_hwc_bwd(ops, rows, O, C, HW, dout, feat, Wp, 2, need, dx_lead=4)
        _, _, dX3u = call_hwc_bwd(ops, rows, O, C, HW, dout, feat, Wp, 3, need, dx_lead=4)
        assert same_bits(dW3, dW1) and same_bits(db3, db1), "which = 1 differs from which = 3"
        assert same_bits(dX3, dX2), "which = 2 differs from which = 3"
        assert same_bits(dX3, dXu) and same_bits(dX3, dX3u), "a dX 8 bytes off differs from the aligned one"
        ops.lds_poison()
        again = call_hwc_bwd(ops, rows, O, C, HW, dout, feat, Wp, 3, need)
        assert all(same_bits(p, q) for p, q in zip((dW3, db3, dX3), again)), "a second call differs"
        if kind == "int":
            assert torch.equal(outs[0], d.out.float()) and torch.equal(outs[1], d.out.float())
            assert torch.equal(dW3, d.dW.float()) and torch.equal(db3[0], d.db.float())
            assert same_bits(dX3, d.dX.float().bfloat16()), "dX is not the RNE bf16 of the exact value"
        else:
            rep.add("forward", ratio(outs[0], d.out, d.outabs), In + sf + 4)
            rep.add("forward single pass", ratio(outs[1], d.out, d.outabs), In + 1 + 4)
            rep.add("dW", ratio(dW3, d.dW, d.dWabs), rows + s1 + 4)
            rep.add("db", ratio(db3[0], d.db, d.dbabs), rows + 4)
            rep.add("dX", ratio(dX3.float(), d.dX, d.dXabs, half_ulp_bf16(d.dX)), O + s2 + 4)
    rep.done()


def test_hwc_weight_batch(ops):
    """Four weights of different (O, C, HW) in one launch (the grid is sized by the largest; the
    blocks past a smaller entry's end must leave): bitwise torch's permute + bf16 cast, nothing
    written past any Wp."""
    g = gen(5)
    shapes = [(5, 8, 3), (132, 24, 5), (1, 1, 1), (260, 64, 25)]
    Ws_ = [gauss(g, (O, C * HW)) for O, C, HW in shapes]
    Wps = [Out2d(1, O * C * HW, dtype=torch.bfloat16) for O, C, HW in shapes]
    P, I = ctypes.c_void_p, ctypes.c_int
    ops.call("avd_linear_weight_hwc", 4, (P * 4)(*[w.data_ptr() for w in Ws_]), (P * 4)(*[w.ptr for w in Wps]),
             (I * 4)(*[s[0] for s in shapes]), (I * 4)(*[s[1] for s in shapes]),
             (I * 4)(*[s[2] for s in shapes]), ops.stream())
    for (O, C, HW), W, Wp in zip(shapes, Ws_, Wps):
        want = W.reshape(O, C, HW).permute(0, 2, 1).reshape(O, C * HW).bfloat16()
        assert same_bits(Wp.take().view(O, C * HW), want), (O, C, HW)
