"""Float64 references, in plain torch on whatever device the inputs live on, of the fused
contrastive cross-entropy avd_xent_fused (csrc/xent.hip): for rows Q [R, P] against columns
K [C, P],

  S[i][j] = inv_t q_i . k_j   (column mask(i) excluded),   loss_i = logsumexp_j S[i][j] - S[i][t(i)]
  dQ, dK  = d (g sum_i loss_i) / d (Q, K)

with row i in half h = i // Bh, i' = i - h Bh, t(i) = tgt[h] + i', mask(i) = msk[h] + i' (msk[h] < 0:
none).

* exact():    float64 autograd of that loss -- the yardstick.
* restated(): the same quantities from their closed forms, in float64, rounding where the kernel
  rounds.  Kept in step with xent.hip:
    - Q and K are rounded to bf16 for both products (stage_block / own_frags: cvt8);
    - S, the row log-sum-exp and L stay unrounded (f32 accumulators; `l` sums the unrounded p);
    - P is rounded to bf16 before P K and P^T Q (pack8).  The row pass rounds exp(S - running
      max) and divides by L afterwards, the column pass rounds exp(S - lse); both are one bf16
      rounding of P's relative precision, which is what is restated;
    - the target score (xent_rows_combine: dot) and the subtracted k_t / q_i terms
      (xent_rows_combine: kv, xent_cols_combine: a.q) come from the UNROUNDED f32 vectors.
  With ``rnd`` the identity it is exact() by another code path (no autograd, no cross_entropy);
  tests/test_xent_ref_cpu.py pins the two to 1e-12.

The band of the GPU tests is 3 x rel-L2(restated, exact) per tensor and per tail slice
(tails()), no floor -- the rule of test_gpu_xattn.py and test_gpu_lstm.py.

One consequence of the kernel's mixed precisions, read from the code: loss_i is a log-sum-exp
of bf16-operand scores minus the f32 target score, so on a converged row (lse ~ the target's
score) it is the rounding error of one scaled score and can come out NEGATIVE, where the true
CE cannot.  A bf16 operand (8 significant bits) is off by at most 2^-8 relative, a score of unit
rows by at most 2^-7 if every element's rounding pulled the same way; the P roundings are in
fact independent, and on a converged row (q ~ k) the error sum_c q_c^2 (dq_c + dk_c) has an rms
of about inv_t 2^-8 sqrt(2 / 3) sqrt(sum_c q_c^4) ~ 0.1 inv_t 2^-8 at P = 128.  The tests hold
every loss row to loss_i >= -(inv_t 2^-8 1.01 + 1e-5) (loss_floor), half the worst case and
some ten standard deviations out.

Also here: the input builders (random / mixed), the product-level restatements of
contrastive.infonce / nt_xent through the float64 l2norm vjp, and the fake world of the
gathered-size tests.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
WEIGHTS = (3.0, 1.7, 1.0, 0.6, 0.3)      # noise weights of the mixed builder (see mixed())


def bf16(x):
    """Round to bf16 (nearest even), back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def index(R, Bh, tgt, msk, device):
    """t [R], m [R] (int64; m = -1: no mask) of the per-half targets / masks."""
    i = torch.arange(R, device=device)
    h = (i >= Bh).long()
    ii = i - h * Bh
    t = torch.tensor(tgt, device=device)[h] + ii
    mo = torch.tensor(msk, device=device)[h]
    m = torch.where(mo >= 0, mo + ii, torch.full_like(mo, -1))
    return t, m


def _masked(S, m):
    has = (m >= 0).nonzero().flatten()
    mask = torch.zeros_like(S, dtype=torch.bool)
    mask[has, m[has]] = True
    return S.masked_fill(mask, float("-inf"))


def exact(q, k, Bh, tgt, msk, inv_t, g, t=None, m=None):
    """float64 autograd -> (loss [R], dq [R, P], dk [C, P]).  t / m: explicit per-row target /
    mask columns instead of the per-half ones (the planted mistakes of the CPU test)."""
    q = q.detach().to(F64).requires_grad_()
    k = k.detach().to(F64).requires_grad_()
    t0, m0 = index(q.shape[0], Bh, tgt, msk, q.device)
    t, m = t0 if t is None else t, m0 if m is None else m
    S = _masked((q @ k.T) * inv_t, m)
    ce = F.cross_entropy(S, t, reduction="none")
    (ce.sum() * g).backward()
    return ce.detach(), q.grad, k.grad


def restated(q, k, Bh, tgt, msk, inv_t, g, rnd=bf16):
    """The closed forms with the kernel's roundings (module docstring) -> (loss, dq, dk)."""
    q, k = q.detach().to(F64), k.detach().to(F64)
    t, m = index(q.shape[0], Bh, tgt, msk, q.device)
    qb, kb = rnd(q), rnd(k)
    S = _masked((qb @ kb.T) * inv_t, m)
    mx = S.max(dim=1, keepdim=True).values
    E = torch.exp(S - mx)
    L = E.sum(dim=1, keepdim=True)
    kt = k[t]
    loss = (mx + torch.log(L)).flatten() - inv_t * (q * kt).sum(dim=1)
    Pb = rnd(E / L)
    dq = g * inv_t * (Pb @ kb - kt)
    dk = (Pb.T @ qb).index_add(0, t, -q) * (g * inv_t)
    return loss, dq, dk


def loss_floor(inv_t):
    """Lower bound of a kernel loss row (module docstring)."""
    return -(inv_t * 2.0 ** -8 * 1.01 + 1e-5)


def rel(a, b):
    return ((a.double() - b).norm() / b.norm()).item()


def tails(loss, dq, dk):
    """The tail slices the band is also applied to: the last 16-row tile of loss and dq (a
    wave's rows in the row pass), the last 32-row block of dk (the column pass's ragged edge)."""
    R, C = dq.shape[0], dk.shape[0]
    r0, c0 = 16 * ((R - 1) // 16), 32 * ((C - 1) // 32)
    return dict(loss_tail=loss[r0:], dq_tail=dq[r0:], dk_tail=dk[c0:])


def named(loss, dq, dk):
    """Every tensor the band applies to."""
    return dict(loss=loss, dq=dq, dk=dk, **tails(loss, dq, dk))


# ---------------------------------------------------------------- inputs
def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def random(R, C, P, seed):
    """Independent random unit rows, f32 on the CPU: logits of std ~ 1.3 at tau = 0.07, a
    near-uniform softmax."""
    g = torch.Generator().manual_seed(seed)
    q = _unit(torch.randn(R, P, generator=g, dtype=F64))
    k = _unit(torch.randn(C, P, generator=g, dtype=F64))
    return q.float(), k.float()


def mixed(R, C, P, Bh, tgt, msk, seed, weights=WEIGHTS):
    """Rows at mixed stages of convergence, f32 on the CPU: row i = normalize(k_t(i) + w noise_i)
    with unit noise (cosine to the positive 1 / sqrt(1 + w^2): 0.32 at w = 3.0 to 0.96 at
    w = 0.3), and the masked own column set to the row itself (its logit inv_t is the row's
    maximum, as in NT-Xent).

    A target may be another row's own column (NT-Xent: rows i' of the two halves are each
    other's positive), so the rows are built half by half: the second half's targets then
    already hold the first half's rows, and the first half's targets are overwritten with the
    second half's rows at exactly the intended cosine (which is symmetric -- iterating the whole
    batch instead drifts every pair towards convergence, until the loss, the band's
    denominator, vanishes).

    w cycles over ``weights`` by the row's distance from the nearer end of its half,
    min(i', Bh - 1 - i'), not by the plain row index: partners share one weight, and the first
    and the last row of a half are unconverged (w = 3.0), so that a tail slice of a single row
    still has a loss to be relative to.

    Where the last column is neither a target nor an own column it is made a hard negative of
    row 0 (cosine 0.71): a far negative of converged rows has a gradient below the rounding
    error, and a kernel that lost the ragged last column would pass unseen."""
    g = torch.Generator().manual_seed(seed)
    k = _unit(torch.randn(C, P, generator=g, dtype=F64)).float()
    noise = _unit(torch.randn(R, P, generator=g, dtype=F64))
    ii = torch.arange(R) % Bh
    w = torch.tensor(weights, dtype=F64)[torch.minimum(ii, Bh - 1 - ii) % len(weights)].unsqueeze(1)
    t, m = index(R, Bh, tgt, msk, "cpu")
    q = torch.empty(R, P)
    for rows in (slice(0, min(R, Bh)), slice(Bh, R)):
        q[rows] = _unit(k[t[rows]].double() + w[rows] * noise[rows]).float()
        has = (m[rows] >= 0).nonzero().flatten()
        k[m[rows][has]] = q[rows][has]
    if C > 1 and not bool((t == C - 1).any() | (m == C - 1).any()):
        k[C - 1] = _unit(q[:1].double() + _unit(torch.randn(1, P, generator=g, dtype=F64))).float()[0]
    return q, k


# ---------------------------------------------------------------- product level
def place(others, mine, r):
    """Rank r's rows at their slot among the other ranks' rows (world 1: ``mine`` alone)."""
    if others is None:
        return mine
    B = mine.shape[0]
    return torch.cat([others[:r * B].to(F64), mine, others[(r + 1) * B:].to(F64)])


def infonce_from_z(zi, za, oi, oa, W, r, tau, fn=restated):
    """contrastive.infonce in float64 from the raw rows zi, za [B, P] of rank r of W (oi, oa
    [W B, P]: the other ranks' unit rows, None for W = 1): fn (exact or restated) gives
    d loss / d(normalised rows); the row and own-column parts are then taken through the float64
    l2norm vjp.  -> parts [2B], loss, dzi, dza, d_oa, d_oi (column gradients [W B, P])."""
    B = zi.shape[0]
    zi = zi.detach().to(F64).requires_grad_()
    za = za.detach().to(F64).requires_grad_()
    ni, na = F.normalize(zi, dim=1), F.normalize(za, dim=1)
    sl = slice(r * B, (r + 1) * B)
    g = 0.5 / B
    l1, dq1, dk1 = fn(ni.detach(), place(oa, na.detach(), r), B, (r * B, 0), (-1, -1), 1.0 / tau, g)
    l2, dq2, dk2 = fn(na.detach(), place(oi, ni.detach(), r), B, (r * B, 0), (-1, -1), 1.0 / tau, g)
    dzi, = torch.autograd.grad(ni, zi, grad_outputs=dq1 + dk2[sl])
    dza, = torch.autograd.grad(na, za, grad_outputs=dq2 + dk1[sl])
    parts = torch.cat([l1, l2])
    return dict(parts=parts, loss=parts.sum().item() * g, dzi=dzi, dza=dza, d_oa=dk1, d_oi=dk2)


def ntxent_from_z(reps, o, W, r, tau, fn=restated):
    """contrastive.nt_xent likewise: reps [2B, P] = [z1; z2] of rank r, o [2 W B, P] = [z1 of
    every rank; z2 of every rank] (None for W = 1).  -> parts [2B], loss, dreps, d_o."""
    B = reps.shape[0] // 2
    WB = W * B
    reps = reps.detach().to(F64).requires_grad_()
    n = F.normalize(reps, dim=1)
    nd = n.detach()
    s1, s2 = slice(r * B, (r + 1) * B), slice(WB + r * B, WB + (r + 1) * B)
    if o is None:
        n_all = nd
    else:
        n_all = torch.cat([place(o[:WB], nd[:B], r), place(o[WB:], nd[B:], r)])
    g = 1.0 / (2 * B)
    parts, dq, dk = fn(nd, n_all, B, (WB + r * B, r * B), (r * B, WB + r * B), 1.0 / tau, g)
    dreps, = torch.autograd.grad(n, reps, grad_outputs=dq + torch.cat([dk[s1], dk[s2]]))
    return dict(parts=parts, loss=parts.sum().item() * g, dreps=dreps, d_o=dk)


class FakeWorld:
    """avdino.dist with a world of W ranks of which this process is ``rank``: the all-gather
    places this rank's rows at its slot among fixed rows of the other ranks, the reduce-scatter
    records the full column gradient and hands back this rank's own slice."""

    def __init__(self, monkeypatch, others, world=8, rank=3):
        from avdino import dist as AD
        self.others = others          # [C, P] f32 unit rows used for the other ranks, per gather
        self.cols = []
        self.W, self.rank = world, rank
        monkeypatch.setattr(AD, "distributed", lambda group=None: True)
        monkeypatch.setattr(AD, "world", lambda group=None: world)
        monkeypatch.setattr(AD, "rank", lambda group=None: rank)
        monkeypatch.setattr(AD, "gather_rows", self.gather)
        monkeypatch.setattr(AD, "scatter_rows_grad", self.scatter)
        self.k = 0

    def gather(self, x, group=None, out=None):
        B = x.shape[0]
        src = self.others[self.k % len(self.others)]
        self.k += 1
        out.copy_(src)
        out[self.rank * B:(self.rank + 1) * B] = x
        return out

    def scatter(self, dx_all, group=None, out=None):
        B = dx_all.shape[0] // self.W
        self.cols.append(dx_all.detach().clone())
        out.copy_(dx_all[self.rank * B:(self.rank + 1) * B])
        return out
