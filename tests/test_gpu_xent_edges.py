"""avd_xent_fused (csrc/xent.hip, the bf16 step's InfoNCE / NT-Xent loss and both gradients) on
edge shapes and on both input regimes, against float64 (tests/xent_ref.py).

Band, per tensor (loss, dq, dk) and per tail slice (the last 16-row tile of loss and dq, the
last 32-row block of dk): rel-L2 to the exact float64 autograd <= 3 x the rel-L2 of the float64
restatement that rounds where the kernel rounds (Q, K and P to bf16; scores, lse and the target
terms unrounded).  No floor.  tests/test_xent_ref_cpu.py shows that a dropped or shifted mask, a
shifted target or a lost last column lands at >= 5x this band on the small cases.

Inputs: `random` (independent unit rows: near-uniform softmax) and `mixed` (rows between cosine
0.32 and 0.96 to their positive, the masked own column the row itself -- the masked logit is
the row's maximum, as in the NT-Xent workload).

Every case also checks
* bitwise determinism over three launches: fresh workspace, the same workspace again (stale
  partials), a workspace pre-filled with NaN -- the result may not depend on what the workspace
  held, so empty splits must publish m = -inf, l = 0, o = 0;
* a sentinel guard: loss, dq, dk and the workspace (sized exactly as xent_fused_ws returns) are
  followed by a sentinel-filled tail that must be untouched;
* the floor loss_i >= -(inv_t 2^-8 1.01 + 1e-5).  The kernel subtracts the f32 target score
  from a log-sum-exp of bf16-operand scores, so a converged row can come out slightly NEGATIVE
  where the reference's CE cannot (derivation: tests/xent_ref.py); the floor bounds that.

Shapes (R, C, P, Bh, tgt, msk): one row, one column, one past the 64-row / 64-column blocks, a
target alone in a ragged last column block, a ragged second half (Bh < R < 2 Bh), and three size
cases that reach split counts the small ones cannot (row pass S = 7; column pass S = 3 and
S = 1, the production split of config 4); the split counts are asserted through the workspace
size, so a retuned split cannot silently void them.

Then the product functions contrastive.infonce / nt_xent on the fused route at small size (a
fake world of 3, world 1, local=True) against float64 from the raw rows through the
normalisation, and P = 64 on the GEMM route.
"""
import functools
import math

import pytest
import torch

from tests import xent_ref as X

pytestmark = pytest.mark.gpu

SENT, PAD = -777.25, 4096
TAU = 0.07

SMALL = [  # R, C, P, Bh, tgt, msk
    (10, 10, 128, 5, (5, 0), (0, 5)),                 # NT-Xent, world 1, tails everywhere
    (6, 24, 256, 3, (15, 3), (3, 15)),                # NT-Xent, a rank of world 4
    (7, 21, 256, 7, (7, 0), (-1, -1)),                # InfoNCE, rank 1 of world 3
    (200, 200, 128, 100, (100, 0), (0, 100)),         # several row / column blocks
    (96, 768, 128, 96, (288, 0), (-1, -1)),           # InfoNCE rank 3 of 8, column splits
    (1, 33, 128, 1, (32, 0), (-1, -1)),               # one row; target alone in a ragged block
    (2, 33, 256, 1, (32, 0), (0, 32)),                # the smallest NT-Xent
    (65, 129, 128, 65, (64, 0), (-1, -1)),            # one past a row block and a column block
    (9, 40, 256, 5, (20, 0), (0, 20)),                # ragged second half (4 of 5 rows)
    (67, 134, 128, 34, (100, 33), (33, 100)),         # ragged second half (33 of 34 rows)
]
ONE = (1, 1, 128, 1, (0, 0), (-1, -1))                # exact is identically zero
ROWS_S7 = (4738, 4769, 128, 4738, (31, 0), (-1, -1))  # row pass S = 7, 75 ragged row blocks
COLS_S3 = (200, 12810, 128, 100, (6405 + 100, 100), (100, 6405 + 100))   # column pass S = 3
COLS_S1 = (6, 32808, 128, 3, (16404 + 3, 3), (3, 16404 + 3))             # column pass S = 1
SIZE = {ROWS_S7: (7, 7), COLS_S3: (8, 3), COLS_S1: (8, 1)}               # (row, column) pass splits


def _id(c):
    return f"R{c[0]}C{c[1]}P{c[2]}"


def xsplit(blocks):
    """xent.hip's xsplit, restated."""
    return max(1, min(8, math.ceil(512 / blocks)))


def scales(case):
    R, Bh = case[0], case[3]
    both = ((1.0 / TAU, 1.0 / R), (2.0, 0.5 / Bh))
    return both[:1] if case in SIZE else both


@functools.lru_cache(maxsize=None)
def reference(case, regime):
    """Inputs (on the device) and, per scale, the float64 exact / restated tensors -- computed
    once; on the CPU but for the size cases."""
    R, C, P, Bh, tgt, msk = case
    seed = R * 1000 + C
    q, k = X.random(R, C, P, seed) if regime == "random" else X.mixed(R, C, P, Bh, tgt, msk, seed)
    qd, kd = q.cuda(), k.cuda()
    qr, kr = (qd, kd) if case in SIZE else (q, k)
    refs = []
    for inv_t, g in scales(case):
        ex = X.named(*X.exact(qr, kr, Bh, tgt, msk, inv_t, g))
        rs = X.named(*X.restated(qr, kr, Bh, tgt, msk, inv_t, g))
        refs.append(({n: v.cuda() for n, v in ex.items()}, {n: X.rel(rs[n], ex[n]) for n in ex if case != ONE}))
    return qd, kd, refs


def guarded(n, fill=SENT):
    """A buffer of n floats followed by a sentinel tail; returns (whole, the n-element view)."""
    buf = torch.full((n + PAD,), SENT, device="cuda")
    buf[:n] = fill
    return buf, buf[:n]


def launch(q, k, case, inv_t, g, ws):
    from avdino import ops
    R, C, P, Bh, tgt, msk = case
    bufs = [guarded(R), guarded(R * P), guarded(C * P)]
    ops.xent_fused(q, k, R, C, P, Bh, tgt, msk, inv_t, g, bufs[0][1], bufs[1][1], bufs[2][1], ws)
    torch.cuda.synchronize()
    for (whole, view) in bufs:
        assert bool((whole[view.numel():] == SENT).all()), "an output's sentinel tail was written"
        assert bool(torch.isfinite(view).all())
    return bufs[0][1], bufs[1][1].view(R, P), bufs[2][1].view(C, P)


def three_launches(q, k, case, inv_t, g):
    """Fresh (sentinel-filled) workspace, the same again, NaN-filled: bit-identical, and the
    workspace's tail untouched.  Returns the first launch's (loss, dq, dk)."""
    from avdino import ops
    need = ops.xent_fused_ws(*case[:3])
    wsb, ws = guarded(need)
    first = launch(q, k, case, inv_t, g, ws)
    again = launch(q, k, case, inv_t, g, ws)
    ws.fill_(float("nan"))
    nan = launch(q, k, case, inv_t, g, ws)
    assert bool((wsb[need:] == SENT).all()), "the workspace's sentinel tail was written"
    for a, b, c in zip(first, again, nan):
        assert torch.equal(a, b), "a second launch over stale partials differs"
        assert torch.equal(a, c), "the result depends on the workspace's contents"
    return first


CASES = [(c, r) for c in SMALL + [COLS_S3, COLS_S1] for r in ("random", "mixed")] + [(ROWS_S7, "random")]


@pytest.mark.parametrize("case,regime", CASES, ids=[f"{_id(c)}-{r}" for c, r in CASES])
def test_xent_fused_band(case, regime, capsys):
    from avdino import ops
    R, C, P = case[:3]
    if case in SIZE:      # the split counts this case is here for, via the workspace layout
        sa, sb = xsplit((R + 63) // 64), xsplit((C + 63) // 64)
        assert (sa, sb) == SIZE[case]
        assert ops.xent_fused_ws(R, C, P) == 2 * sa * R + sa * R * P + R + sb * C * P
    q, k, refs = reference(case, regime)
    for (inv_t, g), (ex, band) in zip(scales(case), refs):
        got = X.named(*three_launches(q, k, case, inv_t, g))
        assert got["loss"].min().item() >= X.loss_floor(inv_t), got["loss"].min().item()
        err = {n: X.rel(got[n], ex[n]) for n in ex}
        with capsys.disabled():
            print(f"\nxent {_id(case)} {regime} 1/t {inv_t:.2f}: min loss {got['loss'].min().item():+.2e}; "
                  + ", ".join(f"{n} {err[n]:.2e} (band {3 * band[n]:.2e})" for n in ex))
        assert all(err[n] <= 3.0 * band[n] for n in ex), (err, band)


@pytest.mark.parametrize("regime", ["random", "mixed"])
def test_xent_fused_one_by_one(regime, capsys):
    """R = C = 1: the softmax is 1 and loss, dq, dk are identically zero in exact arithmetic, so
    there is nothing to be relative to.  What the kernel leaves is the rounding of the one
    score, bounded as the loss floor is (|loss| <= inv_t 2^-8 1.01 + 1e-5), and
    g inv_t (bf16(x) - x) elementwise in the gradients (<= g inv_t 2^-8 1.01 for |x| <= 1)."""
    q, k, refs = reference(ONE, regime)
    for (inv_t, g), (ex, _) in zip(scales(ONE), refs):
        assert all(float(v.abs().max()) == 0.0 for v in ex.values())
        loss, dq, dk = three_launches(q, k, ONE, inv_t, g)
        with capsys.disabled():
            print(f"\nxent R1C1P128 {regime} 1/t {inv_t:.2f}: loss {loss.item():+.2e} (bound {-X.loss_floor(inv_t):.2e}), "
                  f"|dq| {dq.abs().max().item():.2e}, |dk| {dk.abs().max().item():.2e} "
                  f"(bound {g * inv_t * 2.0 ** -8 * 1.01:.2e})")
        assert abs(loss.item()) <= -X.loss_floor(inv_t)
        assert dq.abs().max().item() <= g * inv_t * 2.0 ** -8 * 1.01
        assert dk.abs().max().item() <= g * inv_t * 2.0 ** -8 * 1.01


# ---------------------------------------------------------------- the product functions
def _raw(B, P, seed, regime):
    """Two sets of raw (unnormalised) rows [B, P]; mixed: row i of the second at cosine 0.32 ..
    0.96 to row i of the first."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, P, generator=g, dtype=X.F64)
    b = torch.randn(B, P, generator=g, dtype=X.F64)
    if regime == "mixed":
        w = torch.tensor(X.WEIGHTS, dtype=X.F64)[torch.arange(B) % len(X.WEIGHTS)].unsqueeze(1)
        b = X._unit(a) + w * X._unit(b)
    s = 0.5 + 3 * torch.rand(B, 1, generator=g, dtype=X.F64)
    return (a * 2).float().cuda(), (b * s).float().cuda()


def _others(n, P, seed):
    g = torch.Generator().manual_seed(seed)
    return X._unit(torch.randn(n, P, generator=g, dtype=X.F64)).float().cuda()


def _check(label, err, band, capsys):
    with capsys.disabled():
        print(f"\n{label}: " + ", ".join(f"{n} {err[n]:.2e} (band {3 * band[n]:.2e})" for n in err))
    assert all(err[n] <= 3.0 * band[n] for n in err), (err, band)


WORLDS = [  # world, rank, B, P, local
    (3, 1, 20, 128, False),
    (1, 0, 5, 256, False),          # the local axpy tail
    (3, 1, 5, 128, True),           # local=True inside a world of 3: no exchange
]


@pytest.mark.parametrize("regime", ["random", "mixed"])
@pytest.mark.parametrize("world", WORLDS, ids=["w3r1", "w1", "local"])
def test_infonce_small_fused(monkeypatch, world, regime, capsys):
    from avdino import contrastive, ops
    from avdino.engine import Workspace
    W, r, B, P, local = world
    assert contrastive._fused(ops.GEMM_BF16_MFMA, P)
    zi, za = _raw(B, P, 100 * B + P, regime)
    fw = None
    if W > 1:
        oi, oa = _others(W * B, P, 7), _others(W * B, P, 8)
        fw = X.FakeWorld(monkeypatch, [oi, oa], world=W, rank=r)
    if W == 1 or local:
        W, r, oi, oa = 1, 0, None, None
    ws = Workspace(torch.device("cuda"))
    dzi, dza, parts = torch.empty(B * P, device="cuda"), torch.empty(B * P, device="cuda"), torch.empty(2 * B, device="cuda")
    scale = contrastive.infonce(ws, zi.reshape(-1), za.reshape(-1), B, P, dzi, dza, parts, TAU,
                                ops.GEMM_BF16_MFMA, local=local)
    torch.cuda.synchronize()
    assert scale == 0.5 / B and (fw is None or len(fw.cols) == (0 if local else 2))
    ex = X.infonce_from_z(zi, za, oi, oa, W, r, TAU, fn=X.exact)
    rs = X.infonce_from_z(zi, za, oi, oa, W, r, TAU, fn=X.restated)
    got = dict(parts=parts, dzi=dzi.view(B, P), dza=dza.view(B, P))
    if W > 1:
        keep = torch.ones(W * B, dtype=torch.bool, device="cuda")
        keep[r * B:(r + 1) * B] = False
        got.update(d_oa=fw.cols[0][keep], d_oi=fw.cols[1][keep])
        for d in (ex, rs):
            d.update(d_oa=d["d_oa"][keep], d_oi=d["d_oi"][keep])
    err = {n: X.rel(got[n], ex[n]) for n in got}
    band = {n: X.rel(rs[n], ex[n]) for n in got}
    err["loss"] = abs(parts.double().sum().item() * scale - ex["loss"]) / abs(ex["loss"])
    band["loss"] = abs(rs["loss"] - ex["loss"]) / abs(ex["loss"])
    _check(f"InfoNCE W={W} B={B} P={P} local={local} {regime}", err, band, capsys)


@pytest.mark.parametrize("regime", ["random", "mixed"])
@pytest.mark.parametrize("world", WORLDS, ids=["w3r1", "w1", "local"])
def test_ntxent_small_fused(monkeypatch, world, regime, capsys):
    from avdino import contrastive, ops
    from avdino.engine import Workspace
    W, r, B, P, local = world
    z1, z2 = _raw(B, P, 200 * B + P, regime)
    reps = torch.cat([z1, z2]).contiguous()
    fw = o = None
    if W > 1:
        o = _others(2 * W * B, P, 9)
        fw = X.FakeWorld(monkeypatch, [o[:W * B], o[W * B:]], world=W, rank=r)
    if W == 1 or local:
        W, r, o = 1, 0, None
    ws = Workspace(torch.device("cuda"))
    dreps, parts = torch.empty(2 * B * P, device="cuda"), torch.empty(2 * B, device="cuda")
    scale = contrastive.nt_xent(ws, reps.reshape(-1), B, P, dreps, parts, TAU, ops.GEMM_BF16_MFMA, local=local)
    torch.cuda.synchronize()
    assert scale == 1.0 / (2 * B) and (fw is None or len(fw.cols) == (0 if local else 2))
    ex = X.ntxent_from_z(reps, o, W, r, TAU, fn=X.exact)
    rs = X.ntxent_from_z(reps, o, W, r, TAU, fn=X.restated)
    got = dict(parts=parts, dreps=dreps.view(2 * B, P))
    if W > 1:
        keep = torch.ones(2 * W * B, dtype=torch.bool, device="cuda")
        keep[r * B:(r + 1) * B] = False
        keep[W * B + r * B:W * B + (r + 1) * B] = False
        got["d_o"] = torch.cat(fw.cols)[keep]
        for d in (ex, rs):
            d["d_o"] = d["d_o"][keep]
    err = {n: X.rel(got[n], ex[n]) for n in got}
    band = {n: X.rel(rs[n], ex[n]) for n in got}
    err["loss"] = abs(parts.double().sum().item() * scale - ex["loss"]) / abs(ex["loss"])
    band["loss"] = abs(rs["loss"] - ex["loss"]) / abs(ex["loss"])
    _check(f"NT-Xent W={W} B={B} P={P} local={local} {regime}", err, band, capsys)


def test_p64_takes_the_gemm_route(monkeypatch, capsys):
    """P = 64 is outside the fused kernel (P = 128 / 256): the bf16 step falls to the GEMM +
    softmax-CE route by contrastive._fused, not by an error -- and that route at P = 64 meets
    the f32-route tolerances of tests/test_gpu_contrastive_size.py in f32 mode."""
    from avdino import contrastive, ops
    from avdino.engine import Workspace
    W, r, B, P = 3, 1, 20, 64
    assert not contrastive._fused(ops.GEMM_BF16_MFMA, P) and contrastive._fused(ops.GEMM_BF16_MFMA, 128)
    with pytest.raises(Exception):
        ops.xent_fused_ws(B, W * B, P)
    zi, za = _raw(B, P, 64, "random")
    oi, oa, o = _others(W * B, P, 7), _others(W * B, P, 8), _others(2 * W * B, P, 9)
    fw = X.FakeWorld(monkeypatch, [oi, oa], world=W, rank=r)
    ws = Workspace(torch.device("cuda"))
    dzi, dza, parts = torch.empty(B * P, device="cuda"), torch.empty(B * P, device="cuda"), torch.empty(2 * B, device="cuda")
    scale = contrastive.infonce(ws, zi.reshape(-1), za.reshape(-1), B, P, dzi, dza, parts, TAU, ops.GEMM_F32_MFMA)
    torch.cuda.synchronize()
    ex = X.infonce_from_z(zi, za, oi, oa, W, r, TAU, fn=X.exact)
    keep = torch.ones(W * B, dtype=torch.bool, device="cuda")
    keep[r * B:(r + 1) * B] = False
    err = dict(loss=abs(parts.double().sum().item() * scale - ex["loss"]) / ex["loss"], parts=X.rel(parts, ex["parts"]),
               dzi=X.rel(dzi.view(B, P), ex["dzi"]), dza=X.rel(dza.view(B, P), ex["dza"]),
               col_a=X.rel(fw.cols[0][keep], ex["d_oa"][keep]), col_i=X.rel(fw.cols[1][keep], ex["d_oi"][keep]))
    tol = dict(loss=1e-6, parts=1e-5, dzi=1e-4, dza=1e-4, col_a=1e-4, col_i=1e-4)
    with capsys.disabled():
        print("\nInfoNCE P=64 f32: " + ", ".join(f"{n} {v:.2e} (tol {tol[n]:.0e})" for n, v in err.items()))
    assert all(err[n] <= tol[n] for n in err), (err, tol)

    reps = torch.cat([zi, za]).contiguous()
    fw = X.FakeWorld(monkeypatch, [o[:W * B], o[W * B:]], world=W, rank=r)
    dreps = torch.empty(2 * B * P, device="cuda")
    scale = contrastive.nt_xent(ws, reps.reshape(-1), B, P, dreps, parts, TAU, ops.GEMM_F32_MFMA)
    torch.cuda.synchronize()
    ex = X.ntxent_from_z(reps, o, W, r, TAU, fn=X.exact)
    keep = torch.cat([keep, keep])
    err = dict(loss=abs(parts.double().sum().item() * scale - ex["loss"]) / ex["loss"], parts=X.rel(parts, ex["parts"]),
               dreps=X.rel(dreps.view(2 * B, P), ex["dreps"]), col=X.rel(torch.cat(fw.cols)[keep], ex["d_o"][keep]))
    tol = dict(loss=1e-6, parts=1e-5, dreps=1e-4, col=1e-4)
    with capsys.disabled():
        print("\nNT-Xent P=64 f32: " + ", ".join(f"{n} {v:.2e} (tol {tol[n]:.0e})" for n, v in err.items()))
    assert all(err[n] <= tol[n] for n in err), (err, tol)
