"""tests/xent_ref.py on the CPU: the float64 restatement of avd_xent_fused (xent.hip) is the
exact float64 autograd when its roundings are taken out, and the band the GPU tests build from
it -- 3 x rel-L2(restated, exact) per tensor and tail slice (tests/test_gpu_xent_edges.py) --
has teeth: planted mistakes of the kind a kernel makes (a mask dropped or one column off, one
target one column off, a ragged last column lost) land at >= 5x the band.

Which tensors each mistake must show in:
* mask dropped / shifted (cases with a mask), last row's target shifted: loss, dq and dk as
  whole tensors.  (The tail slices need not: the last row's target need not lie in the last
  column block.)
* last column lost: the dk tail slice (the last 32-column block).  As whole tensors a far
  negative of converged rows is below the rounding error, which is why the GPU test applies
  the band to the tail slices as well.
"""
import pytest
import torch

from tests import xent_ref as X

F64 = torch.float64

SMALL = [  # R, C, P, Bh, tgt, msk: the small cases of tests/test_gpu_xent_edges.py but (1, 1)
    (10, 10, 128, 5, (5, 0), (0, 5)),
    (6, 24, 256, 3, (15, 3), (3, 15)),
    (7, 21, 256, 7, (7, 0), (-1, -1)),
    (200, 200, 128, 100, (100, 0), (0, 100)),
    (96, 768, 128, 96, (288, 0), (-1, -1)),
    (1, 33, 128, 1, (32, 0), (-1, -1)),
    (2, 33, 256, 1, (32, 0), (0, 32)),
    (65, 129, 128, 65, (64, 0), (-1, -1)),
    (9, 40, 256, 5, (20, 0), (0, 20)),
    (67, 134, 128, 34, (100, 33), (33, 100)),
]
ONE = (1, 1, 128, 1, (0, 0), (-1, -1))
IDS = [f"R{c[0]}C{c[1]}P{c[2]}" for c in SMALL]
TEETH = 5.0


def scales(case):
    """(inv_t, g) of the two runs of a small case."""
    R, Bh = case[0], case[3]
    return ((1.0 / 0.07, 1.0 / R), (2.0, 0.5 / Bh))


def inputs(case, regime):
    R, C, P, Bh, tgt, msk = case
    seed = R * 1000 + C
    return X.random(R, C, P, seed) if regime == "random" else X.mixed(R, C, P, Bh, tgt, msk, seed)


def _lost_last_column(q, k, Bh, tgt, msk, inv_t, g):
    """A ragged-tail bug: column C - 1 never enters the log-sum-exp and its dk row is never
    accumulated; the target score (taken from the f32 vectors) is unaffected."""
    q, k = q.to(F64).requires_grad_(), k.to(F64).requires_grad_()
    R, C = q.shape[0], k.shape[0]
    t, m = X.index(R, Bh, tgt, msk, "cpu")
    S = (q @ k.T) * inv_t
    lost = torch.cat([X._masked(S, m)[:, :C - 1], torch.full((R, 1), float("-inf"), dtype=F64)], 1)
    ce = torch.logsumexp(lost, 1) - S[torch.arange(R), t]
    (ce.sum() * g).backward()
    dk = k.grad.clone()
    dk[C - 1] = 0
    return ce.detach(), q.grad, dk


@pytest.mark.parametrize("regime", ["random", "mixed"])
@pytest.mark.parametrize("case", SMALL + [ONE], ids=IDS + ["R1C1P128"])
def test_restated_without_rounding_is_exact(case, regime):
    q, k = inputs(case, regime)
    for inv_t, g in scales(case):
        ex = X.exact(q, k, *case[3:], inv_t, g)
        rs = X.restated(q, k, *case[3:], inv_t, g, rnd=lambda x: x)
        for a, b in zip(rs, ex):
            assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("case", SMALL, ids=IDS)
def test_mixed_inputs_keep_the_band_small(case):
    """The precondition of the band on the mixed inputs: restated vs exact <= 0.1 rel-L2 for every
    tensor and tail slice, so 3x stays far below a missing term (rel-L2 ~ 1)."""
    q, k = inputs(case, "mixed")
    for inv_t, g in scales(case):
        ex = X.named(*X.exact(q, k, *case[3:], inv_t, g))
        rs = X.named(*X.restated(q, k, *case[3:], inv_t, g))
        err = {n: X.rel(rs[n], ex[n]) for n in ex}
        assert all(e <= 0.1 for e in err.values()), err


@pytest.mark.parametrize("regime", ["random", "mixed"])
@pytest.mark.parametrize("case", SMALL, ids=IDS)
def test_band_has_teeth(case, regime):
    R, C, P, Bh, tgt, msk = case
    q, k = inputs(case, regime)
    t, m = X.index(R, Bh, tgt, msk, "cpu")
    for inv_t, g in scales(case):
        ex = X.named(*X.exact(q, k, Bh, tgt, msk, inv_t, g))
        rs = X.named(*X.restated(q, k, Bh, tgt, msk, inv_t, g))
        band = {n: 3.0 * X.rel(rs[n], ex[n]) for n in ex}

        def ratio(res, names):
            got = X.named(*res)
            return {n: X.rel(got[n], ex[n]) / band[n] for n in names}

        planted = {}
        if msk[0] >= 0:
            planted["mask dropped"] = X.exact(q, k, Bh, tgt, (-1, -1), inv_t, g)
            # one column on; one back where that leaves the matrix or hits the target
            m1 = torch.where((m + 1 >= C) | (m + 1 == t), m - 1, m + 1)
            planted["mask shifted"] = X.exact(q, k, Bh, tgt, msk, inv_t, g, m=m1)
        t1 = t.clone()
        t1[-1] = t[-1] + 1 if (t[-1] + 1 < C and t[-1] + 1 != m[-1]) else t[-1] - 1
        planted["last target shifted"] = X.exact(q, k, Bh, tgt, msk, inv_t, g, t=t1)
        for what, res in planted.items():
            r = ratio(res, ("loss", "dq", "dk"))
            assert all(v >= TEETH for v in r.values()), (what, inv_t, r)
        r = ratio(_lost_last_column(q, k, Bh, tgt, msk, inv_t, g), ("dk_tail",))
        assert r["dk_tail"] >= TEETH, ("last column lost", inv_t, r)


def test_bf16_rounding_and_tail_slices():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3], dtype=F64)
    r = X.bf16(x)                              # ties to even; relative error <= 2^-8
    assert r[0] == 1.0 and r[1] == 1.0 + 2.0 ** -6 and abs(r[2] / x[2] - 1) <= 2.0 ** -8
    s = X.tails(torch.zeros(67), torch.zeros(67, 4), torch.zeros(134, 4))
    assert s["loss_tail"].shape[0] == 3 and s["dq_tail"].shape[0] == 3 and s["dk_tail"].shape[0] == 6
    s = X.tails(torch.zeros(64), torch.zeros(64, 4), torch.zeros(64, 4))
    assert s["loss_tail"].shape[0] == 16 and s["dk_tail"].shape[0] == 32
