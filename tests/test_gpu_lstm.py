"""The LSTM recurrence kernels (csrc/lstm.hip: avd_lstm_fwd / avd_lstm_bwd) with the GEMMs around
them -- engine.lstm_forward / lstm_backward, from token rows to the mean-over-time output and to
every gradient -- against torch.nn.LSTM in float64 on the CPU followed by the mean.

Shapes, the smallest that can break it: T in {1, 2, 3, 49 (the multi_lstm image tower), 196 (the
audio tower)}; H every size the dispatcher instantiates (ops.LSTM_HIDDEN).  A wave owns the unit
tiles u = wave, wave + 4 of the NU = H / 16; the bf16 MFMA pads the forward's K = H to a multiple
of 32:
  H = 16   NU 1: wave 0 alone, three waves idle; K padded 16 -> 32
  H = 32   NU 2: waves 2 and 3 idle; no padding
  H = 48   NU 3: wave 3 idle (not a power of two); K padded 48 -> 64
  H = 64   NU 4: exactly one tile per wave; no padding
  H = 80   NU 5: only wave 0 has a second tile; K padded 80 -> 96
  H = 96   NU 6: waves 0 and 1 have a second tile; no padding
  H = 112  NU 7: wave 3 alone has no second tile; K padded 112 -> 128
  H = 128  NU 8: two tiles per wave, the full-residency case; no padding
N in {1, 15, 17, 35} around the kernel's 16-sequence block.  Every (T, H) pair runs, with N cycling
so that every N meets every T and H at least once.  Inputs are random, so asymmetric in time; both
biases are non-zero and different.

f32 band: rel-L2 per tensor <= max(1e-5, 3 x the error of torch's own float32 CPU nn.LSTM against
the same float64 run) -- two independent roundings of the same size.
bf16 band: <= 3 x the deviation, from the unrounded float64 result, of a float64 restatement that
rounds to bf16 where the kernels and their GEMMs do: x, W_ih, W_hh and the fed-back h as matrix
operands in the forward; dG as a matrix operand in the backward (Gx, the cell state, the
activations and the output mean stay unrounded, as in the kernel).
A tensor that is exactly zero in float64 (dW_hh at T = 1: no step has a predecessor) must be
exactly zero."""
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from avdino import ops  # noqa: E402

I = 64
TS, HS, NS = (1, 2, 3, 49, 196), ops.LSTM_HIDDEN, (1, 15, 17, 35)
# N cycles over (T, H) in the order the sizes joined the table, so the earlier cases keep their N
_T_ORDER = (1, 2, 3, 196) + tuple(T for T in TS if T not in (1, 2, 3, 196))
_H_ORDER = (16, 48, 128) + tuple(H for H in HS if H not in (16, 48, 128))
CASES = [(T, H, NS[(_T_ORDER.index(T) + _H_ORDER.index(H)) % 4]) for T in TS for H in HS]
NAMES = [n + s for s in ("", "_reverse")
         for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


def test_case_table_covers_every_size():
    assert set(HS) == set(ops.LSTM_HIDDEN) and len(HS) == 8
    assert {c[0] for c in CASES} == set(TS) and {c[1] for c in CASES} == set(HS)
    assert {c[2] for c in CASES} == set(NS)
    assert {c[:2] for c in CASES} == {(T, H) for T in TS for H in HS} and len(CASES) == 40
    for N in NS:                                      # every N meets every T and every H
        assert {c[0] for c in CASES if c[2] == N} == set(TS), N
        assert {c[1] for c in CASES if c[2] == N} == set(HS), N
    assert ops.LSTM_BLOCK == 16 and NS == (1, ops.LSTM_BLOCK - 1, ops.LSTM_BLOCK + 1, 2 * ops.LSTM_BLOCK + 3)


def inputs(T, H, N):
    g = torch.Generator().manual_seed(1000 * T + 10 * H + N)

    def u(*shape, b=1.0):
        return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * b

    prm = {}
    for n in NAMES:
        if n.startswith("weight_ih"):
            prm[n] = u(4 * H, I, b=I ** -0.5)
        elif n.startswith("weight_hh"):
            prm[n] = u(4 * H, H, b=H ** -0.5)
        else:
            prm[n] = u(4 * H, b=0.3)
    return u(N, T, I), prm, u(N, 2 * H)


def torch_lstm(x, prm, dout, H, dtype):
    """nn.LSTM on the CPU in ``dtype`` -> {"out", "dx", the eight parameter gradients} (float64)."""
    m = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).to(dtype)
    with torch.no_grad():
        for n in NAMES:
            getattr(m, n).copy_(prm[n].to(dtype))
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    out = m(xx)[0].mean(dim=1)
    (out * dout.to(dtype)).sum().backward()
    r = {"out": out.detach().double(), "dx": xx.grad.double()}
    r.update({n: getattr(m, n).grad.double() for n in NAMES})
    return r


class _RoundSTE(torch.autograd.Function):
    """Round to bf16 in the forward (a matrix operand of a bf16 MFMA), identity backward."""

    @staticmethod
    def forward(ctx, v):
        return v.float().bfloat16().double()

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """Identity forward; the gradient is rounded to bf16 (dG as a matrix operand)."""

    @staticmethod
    def forward(ctx, v):
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return g.float().bfloat16().double()


def restated_bf16(x, prm, dout, H):
    """The float64 recurrence with bf16 rounding where the kernels round (module docstring)."""
    rb, rg = _RoundSTE.apply, _RoundGrad.apply
    p = {n: prm[n].clone().requires_grad_(True) for n in NAMES}
    xx = x.clone().requires_grad_(True)
    N, T, _ = x.shape
    halves = []
    for sfx in ("", "_reverse"):
        gx = rb(xx) @ rb(p["weight_ih_l0" + sfx]).t() + (p["bias_ih_l0" + sfx] + p["bias_hh_l0" + sfx])
        whh = rb(p["weight_hh_l0" + sfx])
        h = x.new_zeros(N, H)
        c = x.new_zeros(N, H)
        acc = x.new_zeros(N, H)
        for t in (range(T) if not sfx else reversed(range(T))):
            a = rg(gx[:, t] + rb(h) @ whh.t())
            i, f, g, o = a.split(H, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            acc = acc + h
        halves.append(acc / T)
    out = torch.cat(halves, dim=1)
    (out * dout).sum().backward()
    r = {"out": out.detach(), "dx": xx.grad}
    r.update({n: p[n].grad for n in NAMES})
    return r


@functools.lru_cache(maxsize=None)
def reference(T, H, N):
    """(inputs, float64 result, float32 result, bf16 restatement): computed once per case and
    shared by the tests; never modified."""
    x, prm, dout = inputs(T, H, N)
    return (x, prm, dout), torch_lstm(x, prm, dout, H, torch.float64), \
        torch_lstm(x, prm, dout, H, torch.float32), restated_bf16(x, prm, dout, H)


def gpu_lstm(x, prm, dout, H, bf16, train=True, ws=None, poison=None):
    """engine.lstm_forward (+ lstm_backward when train) on the device -> (result dict of float64
    CPU tensors, workspace)."""
    from avdino import ops
    from avdino.engine import Workspace, lstm_backward, lstm_forward
    N, T, _ = x.shape
    dev = {n: v.float().cuda() for n, v in prm.items()}
    grads = {n: torch.full_like(v, float("nan")) for n, v in dev.items()}
    gm = ops.GEMM_BF16_MFMA if bf16 else ops.GEMM_F32_MFMA
    ws = ws or Workspace(torch.device("cuda"))
    if poison is not None:
        ws.get("k.save", ops.lstm_ws(N, T, H)[0]).fill_(poison)
    xd = x.float().cuda().reshape(-1)
    out, save = lstm_forward(ws, "k", xd, N, T, H, dev.__getitem__, gm, bf16, train)
    r = {"out": out.double().cpu()}
    if train:
        dx = lstm_backward(ws, xd, save, dout.float().cuda().reshape(-1), N, T, H, dev.__getitem__,
                           grads.__getitem__, gm, bf16)
        r["dx"] = dx.view(N, T, I).double().cpu()
        r.update({n: g.double().cpu() for n, g in grads.items()})
    torch.cuda.synchronize()
    return r, ws


def rel(a, b):
    return float((a - b).norm() / b.norm())


def check(got, ref, yard, factor, floor):
    """Every tensor of ``got`` within max(floor, factor x yard's error) of ref, rel-L2."""
    report = {}
    for k, r in ref.items():
        if float(r.norm()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
            continue
        e, band = rel(got[k], r), max(floor, factor * rel(yard[k], r))
        report[k] = (e, band)
    print({k: f"{e:.2e}/{b:.2e}" for k, (e, b) in report.items()})
    bad = {k: v for k, v in report.items() if not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("T,H,N", CASES)
def test_f32_matches_float64_lstm(T, H, N):
    (x, prm, dout), r64, r32, _ = reference(T, H, N)
    got, _ = gpu_lstm(x, prm, dout, H, False)
    assert set(got) == set(r64) and len(got) == 10
    check(got, r64, r32, 3.0, 1e-5)


@pytest.mark.parametrize("T,H,N", CASES)
def test_bf16_within_three_times_the_restated_rounding(T, H, N):
    (x, prm, dout), r64, _, rbf = reference(T, H, N)
    got, _ = gpu_lstm(x, prm, dout, H, True)
    check(got, r64, rbf, 3.0, 0.0)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("T,H,N", [(3, 48, 35), (196, 128, 17), (2, 16, 1), (49, 80, 17), (3, 112, 35)])
def test_runs_are_bitwise_reproducible(T, H, N, bf16):
    (x, prm, dout), _, _, _ = reference(T, H, N)
    a, ws = gpu_lstm(x, prm, dout, H, bf16)
    b, _ = gpu_lstm(x, prm, dout, H, bf16, ws=ws)
    c, _ = gpu_lstm(x, prm, dout, H, bf16)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("T,H,N", [(3, 48, 35), (196, 128, 17), (49, 80, 17), (3, 112, 35)])
def test_no_save_is_bitwise_the_same_and_leaves_the_buffer_alone(T, H, N, bf16):
    from avdino import ops
    (x, prm, dout), _, _, _ = reference(T, H, N)
    a, _ = gpu_lstm(x, prm, dout, H, bf16)
    b, ws = gpu_lstm(x, prm, dout, H, bf16, train=False, poison=-7.25)
    assert torch.equal(a["out"], b["out"])
    save = ws.get("k.save", ops.lstm_ws(N, T, H)[0])
    assert bool((save == -7.25).all())
