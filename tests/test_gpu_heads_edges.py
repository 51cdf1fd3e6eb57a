"""Edge-shape parity of the loss, optimiser, eval, staging and dense activation kernels
(csrc/loss.hip, optim.hip, eval.hip, stage.hip, bn.hip) against the float64 oracle.

Every case
  * writes into outputs pre-filled with NaN (integers: a negative pattern) that are followed by
    a guard region of sentinels, which must come back untouched;
  * is compared per row (relative L2 of each row against that row of the reference), so the
    1e12-times larger gradient of a zero-norm row cannot hide its neighbours;
  * runs a second time after ops.lds_poison() and must reproduce every output bit.

Bounds are those test_gpu_ops.py asserts for the same kernel and quantity.  Where a row needs
more (a three-step Adam update of a single element, say), the band is
4x the error of a float32 numpy evaluation of the oracle's own formula against the float64
oracle on the same inputs, and the measured error and the band are printed.  Scalars the
kernels take as f32 (momenta, betas, eps) are given to the oracle at their f32 value.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import numpy_oracle as O  # noqa: E402

GUARD = 64
F_SENT = -1024.0               # exact in f32 and bf16
I_FILL = -0x0123456789ABCDE
I_SENT = -0x5A5A5A5A5A5A5A5
U = 2.0 ** -24                 # f32 unit roundoff


def f32(x):
    """The f32 value of a scalar the kernel receives as float."""
    return float(np.float32(x))


@pytest.fixture(scope="module")
def ops():
    from avdino import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


class Buf:
    """n elements at a 16-byte-aligned offset ``lead`` of a larger allocation, NaN (integers:
    I_FILL) or ``init``, with sentinels before and after."""

    def __init__(self, n, dtype=torch.float32, init=None, lead=0):
        self.n, self.lead, self.fp = n, lead, dtype.is_floating_point
        self.full = torch.empty(lead + n + GUARD, dtype=dtype, device="cuda")
        self.full.fill_(float("nan") if self.fp else I_FILL)
        self.sent = F_SENT if self.fp else I_SENT
        self.full[:lead] = self.sent
        self.full[lead + n:] = self.sent
        self.v = self.full[lead:lead + n]
        if init is not None:
            self.v.copy_(dev(np.asarray(init).ravel(), dtype))

    def check(self):
        assert bool((self.full[:self.lead] == self.sent).all()), "write before the buffer"
        assert bool((self.full[self.lead + self.n:] == self.sent).all()), "write past the buffer"

    def np(self):
        a = self.v.detach().cpu()
        return a.double().numpy() if self.fp else a.numpy()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def twice(ops, run):
    """run() -> Bufs; again after the LDS poison: same bits, guards intact.  Returns the first."""
    a = run()
    torch.cuda.synchronize()
    ops.lds_poison()
    b = run()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        if x is None:
            continue
        x.check()
        y.check()
        assert same_bits(x.full, y.full), "result changed after the LDS poison"
    return a


def row_rel(got, ref):
    """Relative L2 error of each row; a row whose reference is exactly zero must be zero."""
    got = np.asarray(got, np.float64).reshape(ref.shape[0], -1)
    ref = np.asarray(ref, np.float64).reshape(ref.shape[0], -1)
    d = np.linalg.norm(got - ref, axis=1)
    r = np.linalg.norm(ref, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(r > 0, d / np.where(r > 0, r, 1.0), np.where(d == 0, 0.0, np.inf))


def norm_grad_rows(capsys, what, got, ref, f32ref, zero_rows, cond):
    """Rows of a gradient through a normalisation, dx = (g - y (y.g)) / d: per-row relative 1e-5
    (f32-oracle band where needed), except the rows in ``zero_rows``, whose true value is exactly
    zero because g is parallel to y (the partner of a zero row in the MSE loss; every row at
    P = 1).  There the float64 reference holds only its own rounding noise and a relative error
    means nothing: those rows alone are held to the absolute 16 * 2^-24 * cond, cond = |g| / d
    being the norm of the two vectors the row is the difference of (16 f32 roundings of them)."""
    got = np.asarray(got, np.float64).reshape(ref.shape[0], -1)
    zero_rows = np.asarray(zero_rows, bool)
    keep = ~zero_rows
    if keep.any():
        within(capsys, what, row_rel(got[keep], ref[keep]), 1e-5,
               lambda: row_rel(np.asarray(f32ref()).reshape(ref.shape)[keep], ref[keep]))
    if zero_rows.any():
        err = np.linalg.norm(got[zero_rows] - ref[zero_rows], axis=1)
        assert not np.isnan(err).any(), f"{what}: NaN (an element was not written)"
        assert (err <= 16 * U * np.asarray(cond, np.float64)[zero_rows]).all(), (what, err)


def within(capsys, what, err, bound, band=None):
    """err <= bound everywhere; else, with ``band`` (a callable giving the f32-oracle error of
    the same quantity), err <= max(bound, 4 band), printed."""
    err = np.atleast_1d(np.asarray(err, np.float64))
    assert not np.isnan(err).any(), f"{what}: NaN (an element was not written)"
    if (err <= bound).all():
        return
    assert band is not None, f"{what}: {err.max():.3e} > {bound:.3e}"
    tol = np.maximum(bound, 4.0 * np.atleast_1d(np.asarray(band(), np.float64)))
    with capsys.disabled():
        i = int(np.argmax(err - tol))
        print(f"\n[heads-edges] {what}: measured {err.max():.3e} (row {i}: {err[i]:.3e}), "
              f"fixed bound {bound:.1e}, f32-oracle band x4 {tol[i]:.3e}")
    assert (err <= tol).all(), f"{what}: {err.max():.3e} exceeds the band (max {tol.max():.3e})"


P_LIST = [1, 63, 64, 65, 300, 512]


# ------------------------------------------------------------------------------- DINO loss
def _dino_inputs(V, T, B, P):
    g = np.random.default_rng(1000 * P + 100 * V + 10 * T + B)
    nS, nT = V * B, T * B
    s = g.normal(size=(nS, P)).astype(np.float32)
    t = g.normal(size=(nT, P)).astype(np.float32)
    center = g.normal(scale=0.1, size=P).astype(np.float32)
    if nS >= 4:
        s[1] = 0.0                       # zero-norm student row
        s[2] *= np.float32(1e-3)
        s[nS - 1] *= np.float32(1e3)
    if nT >= 2:
        t[nT - 1] = center               # zero-norm teacher row after centring
    return s.reshape(V, B, P), t.reshape(T, B, P), center


def _dino_ref(s, tc, tau_s, tau_t, ct):
    """(loss, per-row loss parts [V*B], ds [V*B, P]) from the oracle's pieces, in s.dtype."""
    V, B, P = s.shape
    T = tc.shape[0]
    loss, ds = O.dino_loss(s, tc, tau_s, tau_t, center_teacher=ct)
    sn, _ = O.l2norm_fwd(s)
    tn, _ = O.l2norm_fwd(tc)
    if ct:
        tn = tn - tn.mean(axis=1, keepdims=True)
    ptsum = O.softmax(tn / tau_t).sum(axis=0)
    parts = -(ptsum[None] * O.log_softmax(sn / tau_s)).sum(axis=-1) / (B * V * T)
    return loss, parts.reshape(-1), ds.reshape(V * B, P)


@pytest.mark.parametrize("center_teacher", [False, True])
@pytest.mark.parametrize("V,T,B", [(3, 2, 5), (1, 1, 1), (6, 2, 7)])
@pytest.mark.parametrize("P", P_LIST)
def test_dino_loss_edges(ops, capsys, P, V, T, B, center_teacher):
    s, t_raw, center = _dino_inputs(V, T, B, P)
    tau_s, tau_t, cm = 0.1, 0.04, 0.9
    tc = t_raw - center                                   # f32, as the kernel forms it
    loss, parts_ref, ds_ref = _dino_ref(s.astype(np.float64), tc.astype(np.float64), tau_s, tau_t,
                                        center_teacher)
    assert abs(parts_ref.sum() - loss) < 1e-12
    ts, tt, tcen = dev(s), dev(t_raw), dev(center)

    def run():
        parts, ds, cn = Buf(V * B), Buf(V * B * P), Buf(P)
        work = Buf((B + T * B) * P)
        ops.dino_loss(ts, tt, tcen, V, T, B, P, tau_s, tau_t, cm, center_teacher, parts.v, ds.v,
                      cn.v, work.v)
        return parts, ds, cn, work

    parts, ds, cn, _ = twice(ops, run)

    def f32ref():
        return _dino_ref(s, tc, tau_s, tau_t, center_teacher)

    tag = f"dino P={P} VTB={V, T, B} ct={int(center_teacher)}"
    within(capsys, tag + " loss_parts", np.abs(parts.np() - parts_ref), 1e-5,
           lambda: np.abs(f32ref()[1].astype(np.float64) - parts_ref))
    within(capsys, tag + " ds", row_rel(ds.np(), ds_ref), 1e-5,
           lambda: row_rel(f32ref()[2], ds_ref))
    cmf = f32(cm)
    cref = cmf * center.astype(np.float64) + (1 - cmf) * t_raw.reshape(-1, P).astype(np.float64).mean(0)
    within(capsys, tag + " center_new",
           np.linalg.norm(cn.np() - cref) / max(np.linalg.norm(cref), 1e-30), 1e-6)


# ------------------------------------------------------------------------- MSE, L2 normalise
def _rows_inputs(rows, P, seed):
    g = np.random.default_rng(seed + 1000 * P + rows)
    a = g.normal(size=(rows, P)).astype(np.float32)
    b = g.normal(size=(rows, P)).astype(np.float32)
    if rows >= 5:
        a[1] = 0.0
        b[3] = 0.0
    return a, b


def _mse_ref(a, b):
    loss, da, db = O.mse_loss(a, b)
    an, ca = O.l2norm_fwd(a)
    bn, cb = O.l2norm_fwd(b)
    parts = ((an - bn) ** 2).sum(axis=1) / a.size
    gn = np.linalg.norm(2.0 * (an - bn) / a.size, axis=1)       # the normalisations' incoming gradient
    return loss, parts, da, db, gn / ca[2].ravel(), gn / cb[2].ravel()


@pytest.mark.parametrize("rows", [1, 5, 4097])
@pytest.mark.parametrize("P", P_LIST)
def test_mse_loss_edges(ops, capsys, P, rows):
    a, b = _rows_inputs(rows, P, 11)
    loss, parts_ref, da_ref, db_ref, ka, kb = _mse_ref(a.astype(np.float64), b.astype(np.float64))
    assert abs(parts_ref.sum() - loss) < 1e-12
    ta, tb = dev(a), dev(b)

    def run():
        parts, da, db = Buf(rows), Buf(rows * P), Buf(rows * P)
        ops.mse_loss(ta, tb, rows, P, parts.v, da.v, db.v)
        return parts, da, db

    parts, da, db = twice(ops, run)
    tag = f"mse P={P} rows={rows}"
    assert abs(parts.np().sum() - loss) < 1e-6
    # each part is a sum of <= 512 non-negative f32 terms of normalised rows: the gradients' bound
    within(capsys, tag + " loss_parts", np.abs(parts.np() - parts_ref) / np.maximum(parts_ref, 1e-300),
           1e-5, lambda: np.abs(_mse_ref(a, b)[1] - parts_ref) / np.maximum(parts_ref, 1e-300))
    # exactly-zero gradient rows: every non-zero row at P = 1, and the partner of a zero row
    za, zb = ~a.any(axis=1), ~b.any(axis=1)
    norm_grad_rows(capsys, tag + " da", da.np(), da_ref, lambda: _mse_ref(a, b)[2],
                   ~za & (zb | (P == 1)), ka)
    norm_grad_rows(capsys, tag + " db", db.np(), db_ref, lambda: _mse_ref(a, b)[3],
                   ~zb & (za | (P == 1)), kb)


@pytest.mark.parametrize("rows", [1, 5, 4097])
@pytest.mark.parametrize("P", P_LIST)
def test_l2norm_edges(ops, capsys, P, rows):
    x, dy = _rows_inputs(rows, P, 13)
    if rows >= 5:
        dy[3] = np.random.default_rng(3).normal(size=P).astype(np.float32)   # zero rows in x only
        x[3] = 0.0
    y_ref, cache = O.l2norm_fwd(x.astype(np.float64))
    dx_ref = O.l2norm_bwd(dy.astype(np.float64), cache)
    tx, tdy = dev(x), dev(dy)

    def run():
        y, norms, dx = Buf(rows * P), Buf(rows), Buf(rows * P)
        ops.l2norm_fwd(tx, y.v, norms.v, rows, P)
        ops.l2norm_bwd(y.v, norms.v, tdy, dx.v, rows, P)
        return y, norms, dx

    y, norms, dx = twice(ops, run)

    def f32ref():
        yy, c = O.l2norm_fwd(x)
        return yy, c[1].reshape(-1), O.l2norm_bwd(dy, c)

    tag = f"l2norm P={P} rows={rows}"
    # <= 8 serial + 6 tree additions of squares (halved by the square root), the root, the
    # reciprocal and the product: <= 10 roundings of 2^-24 = 6e-7
    within(capsys, tag + " y", row_rel(y.np(), y_ref), 1e-6, lambda: row_rel(f32ref()[0], y_ref))
    n_ref = cache[1].reshape(-1)
    within(capsys, tag + " norms", np.abs(norms.np() - n_ref) / np.maximum(n_ref, 1e-300), 1e-6,
           lambda: np.abs(f32ref()[1] - n_ref) / np.maximum(n_ref, 1e-300))
    kx = np.linalg.norm(dy.astype(np.float64), axis=1) / cache[2].ravel()
    norm_grad_rows(capsys, tag + " dx", dx.np(), dx_ref, lambda: f32ref()[2],
                   x.any(axis=1) & (P == 1), kx)


# ---------------------------------------------------------------------- softmax cross-entropy
def _xent_targets(R, C, mode, tgt_off, mask_off, g):
    if mode == 0:
        t = g.integers(0, C, R)
        if mask_off is not None:                       # a target is never the masked column
            t = np.where(t == np.arange(R) + mask_off, (t + 1) % C, t)
        return t
    if mode == 1:
        return np.arange(R) + tgt_off
    return (np.arange(R) + R // 2) % R


def _xent_ref(logits, tgt, mask_off, gscale):
    """(per-row loss, dlogits) of the logical [R, C] matrix in logits.dtype."""
    R, C = logits.shape
    full = logits.copy()
    if mask_off is not None:
        m = np.arange(R) + mask_off
        ok = m < C
        full[np.arange(R)[ok], m[ok]] = -np.inf
    ls = O.log_softmax(full)
    _, d = O.cross_entropy(full, tgt)                  # (softmax - onehot) / R
    return -ls[np.arange(R), tgt], d * (R * gscale)


XENT_CASES = [
    # ldp / lddp: padding columns of ld / ldd; acc: accumulate onto non-zero dlogits; grad=False:
    # dlogits None; big: logits ~ N(0, 30^2) with one row shifted by +1e4
    dict(R=5, C=1, mode=0),
    dict(R=3, C=63, mode=0, ldp=3, lddp=5),
    dict(R=5, C=64, mode=1, tgt_off=59),
    dict(R=5, C=64, mode=0, grad=False),
    dict(R=5, C=65, mode=0, mask_off=62, ldp=1),
    dict(R=5, C=65, mode=0, col_major=True, ldp=2, lddp=1),
    dict(R=5, C=65, mode=1, tgt_off=3, col_major=True, ldp=2, lddp=3, acc=True),
    dict(R=7, C=130, mode=1, tgt_off=100, mask_off=64, ldp=10, lddp=3, acc=True),
    dict(R=7, C=130, mode=0, mask_off=64),
    dict(R=4097, C=10, mode=0),
    dict(R=4097, C=10, mode=0, ldp=2, lddp=6, acc=True),
    dict(R=130, C=130, mode=2, mask_off=0),
    dict(R=130, C=130, mode=2, mask_off=0, col_major=True, ldp=2, lddp=2, acc=True),
    dict(R=5, C=65, mode=0, big=True),
    dict(R=7, C=130, mode=1, tgt_off=64, big=True, ldp=1, lddp=1),
]


@pytest.mark.parametrize("case", XENT_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_softmax_xent_edges(ops, capsys, case):
    R, C, mode = case["R"], case["C"], case["mode"]
    tgt_off, mask_off = case.get("tgt_off", 0), case.get("mask_off")
    cm, acc, grad, big = case.get("col_major", False), case.get("acc", False), case.get("grad", True), case.get("big", False)
    lead_n = R if cm else C                      # elements one leading step spans
    nlead = C if cm else R                       # number of leading steps
    ld, ldd = lead_n + case.get("ldp", 0), lead_n + case.get("lddp", 0)
    g = np.random.default_rng(7 * R + C + mode)
    logits = g.normal(size=(R, C)).astype(np.float32)
    if big:
        logits = (30.0 * logits).astype(np.float32)
        logits[R // 2] += np.float32(1e4)
    tgt = _xent_targets(R, C, mode, tgt_off, mask_off, g)
    gscale = 1.0 / R                             # a power of two or not: applied in f32 either way
    loss_ref, d_ref = _xent_ref(logits.astype(np.float64), tgt, mask_off, f32(gscale))
    init = g.normal(size=(nlead, ldd)).astype(np.float32)
    if acc:
        d_ref = d_ref + (init.T if cm else init)[:R, :C]

    stored = np.full((nlead, ld), np.float32(777.0))       # padding a read would notice
    stored[:, :lead_n] = logits.T if cm else logits
    tl = dev(stored)
    tt = dev(tgt.astype(np.int64)) if mode == 0 else None

    def run():
        lp = Buf(R)
        dl = Buf(nlead * ldd, init=init if acc else None) if grad else None
        ops.softmax_xent(tl, ld, R, C, tt, mode, cm, False, gscale, lp.v, dl.v if grad else None, ldd,
                         acc, tgt_off=tgt_off, mask_off=mask_off)
        return lp, dl

    lp, dl = twice(ops, run)
    tag = "xent " + " ".join(f"{k}={v}" for k, v in case.items())

    def f32ref():
        l32, d32 = _xent_ref(logits, tgt, mask_off, np.float32(gscale))
        return l32, (d32 + (init.T if cm else init)[:R, :C]) if acc else d32

    if big:
        bound = 8 * 2.0 ** -23 * np.maximum(1.0, np.abs(logits).max(axis=1))
        err = np.abs(lp.np() - loss_ref)
        assert not np.isnan(err).any() and (err <= bound).all(), (tag, err, bound)
    else:
        fixed = 1e-6 if mode == 0 and mask_off is None else 1e-5
        within(capsys, tag + " loss", np.abs(lp.np() - loss_ref), fixed,
               lambda: np.abs(f32ref()[0].astype(np.float64) - loss_ref))
    if not grad:
        return
    got = dl.np().reshape(nlead, ldd)
    pad = dl.v.reshape(nlead, ldd)[:, lead_n:]
    if acc:
        assert same_bits(pad, dev(init[:, lead_n:])), "padding columns of dlogits were written"
    else:
        assert bool(torch.isnan(pad).all()), "padding columns of dlogits were written"
    got = (got[:, :lead_n].T if cm else got[:, :lead_n])
    # large logits included: the gradient keeps the table bound (the kernel subtracts the row
    # maximum before log se, so the softmax does not carry the rounding of lse)
    fixed = 1e-6 if mode == 0 and mask_off is None else 1e-5
    within(capsys, tag + " dlogits", row_rel(got, d_ref), fixed, lambda: row_rel(f32ref()[1], d_ref))


# ----------------------------------------------------------------------------------- argmax
def _argmax_rows(R, C, g):
    """Rows cycling through the tie patterns (row % 8); returns logits [max(R, 8), C].  R = 5
    sees patterns 0..4 (every tie the kernels' contract names); patterns 5..7 run at R = 1
    (one launch per pattern) and R = 4099."""
    n = max(R, 8)
    x = g.normal(size=(n, C)).astype(np.float32)
    top = np.float32(9.0)
    for r in range(n):
        k = r % 8
        if k == 0:
            x[r] = -np.inf                                   # all -inf: index 0
        elif k == 1 and C > 67:
            x[r, 3] = x[r, 67] = top                         # same lane, two passes
        elif k == 2 and C > 6:
            x[r, 5] = x[r, 6] = top                          # adjacent lanes
        elif k == 3:
            x[r, 0] = x[r, C - 1] = top                      # first and last column
        elif k == 4:
            x[r] = np.float32(0.5)                           # all equal
        elif k == 5 and C > 67:
            x[r, 67] = x[r, 4] = top                         # later pass, earlier lane vs column 4
        elif k == 6:
            x[r] = -np.inf
            x[r, C // 2] = np.float32(-3.0)                  # one finite entry
    return x


@pytest.mark.parametrize("R", [1, 5, 4099])
@pytest.mark.parametrize("C", [1, 10, 64, 65, 200])
def test_argmax_rows_and_correct_edges(ops, C, R):
    g = np.random.default_rng(31 * C + R)
    x = _argmax_rows(R, C, g)
    ld = C + 3 if R != 1 else C + 1
    stored = np.full((x.shape[0], ld), np.float32(np.inf))   # padding: a read would win the argmax
    stored[:, :C] = x
    want = np.argmax(x, axis=1)
    tgt = np.where(np.arange(x.shape[0]) % 2 == 0, want, (want + 1) % C)
    tx, tt = dev(stored), dev(tgt.astype(np.int64))
    starts = range(8) if R == 1 else [0]                     # R = 1: every pattern as its own launch
    for r0 in starts:
        def run():
            idx, cor = Buf(R, torch.int64), Buf(R)
            ops.argmax_rows(tx[r0:], ld, R, C, idx.v)
            ops.argmax_correct(tx[r0:], ld, R, C, tt[r0:], cor.v)
            return idx, cor

        idx, cor = twice(ops, run)
        assert np.array_equal(idx.np(), want[r0:r0 + R]), (r0, idx.np()[:8], want[r0:r0 + 8])
        assert np.array_equal(cor.np(), (want == tgt)[r0:r0 + R].astype(np.float64)), r0


# ----------------------------------------------------------------------- cosine consistency
def _cos_ref(emb, alpha):
    V, B, D = emb.shape
    loss, d = O.cosine_consistency_loss(emb)
    n, _ = O.l2norm_fwd(emb)
    parts = np.zeros(B, emb.dtype)
    for i in range(V):
        for j in range(i + 1, V):
            parts += (1 - (n[i] * n[j]).sum(-1)) ** 2
    count = V * (V - 1) // 2
    return loss, alpha * parts / (count * B), alpha * d.reshape(V * B, D)


@pytest.mark.parametrize("V,B,D", [(2, 1, 1), (3, 3, 63), (5, 3, 65), (8, 2, 256), (32, 1, 300)])
def test_cosine_consistency_edges(ops, capsys, V, B, D):
    g = np.random.default_rng(V * 1000 + B * 100 + D)
    emb = g.normal(size=(V, B, D)).astype(np.float32)
    emb[1, 0] = 0.0                                          # one zero view row
    alpha = 0.7
    init = (0.01 * g.normal(size=(V * B, D))).astype(np.float32)
    loss, parts_ref, d_ref = _cos_ref(emb.astype(np.float64), f32(alpha))
    assert abs(parts_ref.sum() - f32(alpha) * loss) < 1e-12
    te = dev(emb)

    def run():
        lp, de = Buf(B), Buf(V * B * D, init=init)
        lp_only, de_only = Buf(B), Buf(V * B * D, init=init)
        ops.cosine_consistency(te, V, B, D, alpha, lp.v, de.v)
        ops.cosine_consistency(te, V, B, D, alpha, lp_only.v, None)
        ops.cosine_consistency(te, V, B, D, alpha, None, de_only.v)
        return lp, de, lp_only, de_only

    lp, de, lp_only, de_only = twice(ops, run)
    assert same_bits(lp.v, lp_only.v) and same_bits(de.v, de_only.v)

    def f32ref():
        _, p32, d32 = _cos_ref(emb, np.float32(alpha))
        return p32, d32 + init

    tag = f"cosine V={V} B={B} D={D}"
    within(capsys, tag + " loss_parts", np.abs(lp.np() - parts_ref), 1e-5,
           lambda: np.abs(f32ref()[0].astype(np.float64) - parts_ref))
    total = d_ref + init
    within(capsys, tag + " demb", row_rel(de.np(), total), 1e-5, lambda: row_rel(f32ref()[1], total))


# ---------------------------------------------------------------- flat updates: EMA, axpy, Adam
N_LIST = [1, 3, 4, 5, 1027, 4 * 1024 * 4096 + 1027]
LEAD = 4                                   # operands start 16 bytes into their allocation


def chunk_rel(got, ref, chunk=1 << 20):
    """Relative L2 per chunk of 2^20 elements and of the last 1030 (the last grid-stride trip
    and the scalar tail), so a handful of wrong elements cannot drown in 16M right ones."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    cuts = list(range(0, got.size, chunk)) + [max(got.size - 1030, 0)]
    out = []
    for c in cuts:
        e = min(c + chunk, got.size)
        out.append(np.linalg.norm(got[c:e] - ref[c:e]) / max(np.linalg.norm(ref[c:e]), 1e-300))
    return np.array(out)


def _flat(n, seed, k):
    g = np.random.default_rng(seed + n % 9973)
    return [g.standard_normal(n, dtype=np.float32) for _ in range(k)]


@pytest.mark.parametrize("n", N_LIST)
def test_ema_axpy_edges(ops, capsys, n):
    t, s, y = _flat(n, 41, 3)
    m, a = 0.996, -0.37
    ema_ref = O.ema(t.astype(np.float64), s.astype(np.float64), f32(m))
    axpy_ref = y.astype(np.float64) + f32(a) * s.astype(np.float64)

    def run():
        bt, bs, by = (Buf(n, init=v, lead=LEAD) for v in (t, s, y))
        ops.ema(bt.v, bs.v, n, m)
        ops.axpy(by.v, bs.v, a)
        return bt, bs, by

    bt, bs, by = twice(ops, run)
    assert same_bits(bs.v, dev(s)), "the source operand was written"
    within(capsys, f"ema n={n}", chunk_rel(bt.np(), ema_ref), 1e-7,
           lambda: chunk_rel(O.ema(t, s, np.float32(m)), ema_ref))
    within(capsys, f"axpy n={n}", chunk_rel(by.np(), axpy_ref), 1e-7,
           lambda: chunk_rel(y + np.float32(a) * s, axpy_ref))


HP = dict(lr=f32(1e-3), wd=f32(1e-2), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))


def _adam_oracle(decoupled, p, gr, steps, dtype):
    step_fn = O.adamw_step if decoupled else O.adam_step
    p, gr = p.astype(dtype), gr.astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step in steps:
        p, m, v = step_fn(p, gr, m, v, step, HP["lr"], HP["wd"], HP["b1"], HP["b2"], HP["eps"])
    return p, m, v


def _check_pmv(capsys, tag, got, ref, f32ref):
    """p at test_gpu_ops' 1e-7; m and v (two or three f32 products and a sum per step, no bound
    of record) at the same figure, with the f32-oracle band where a tiny vector needs it."""
    for i, name in enumerate("pmv"):
        within(capsys, f"{tag} {name}", chunk_rel(got[i], ref[i]), 1e-7,
               lambda i=i: chunk_rel(f32ref()[i], ref[i]))


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("n", N_LIST)
def test_adam_edges(ops, capsys, n, decoupled):
    p, gr = _flat(n, 43 + decoupled, 2)
    steps = (1, 2, 3)
    ref = _adam_oracle(decoupled, p, gr, steps, np.float64)
    fn = ops.adamw if decoupled else ops.adam

    def run():
        bp, bg = Buf(n, init=p, lead=LEAD), Buf(n, init=gr, lead=LEAD)
        bm, bv = Buf(n, init=np.zeros(1, np.float32), lead=LEAD), Buf(n, init=np.zeros(1, np.float32), lead=LEAD)
        for step in steps:
            fn(bp.v, bg.v, bm.v, bv.v, n, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"],
               1 - HP["b1"] ** step, 1 - HP["b2"] ** step)
        return bp, bm, bv, bg

    bp, bm, bv, bg = twice(ops, run)
    assert same_bits(bg.v, dev(gr)), "the gradient was written"
    _check_pmv(capsys, f"{'adamw' if decoupled else 'adam'} n={n}", (bp.np(), bm.np(), bv.np()), ref,
               lambda: _adam_oracle(decoupled, p, gr, steps, np.float32))


@pytest.mark.parametrize("with_seed", [True, False])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam_dev", "adamw_dev"])
@pytest.mark.parametrize("t0", [0, 999])
def test_step_begin_and_adam_dev(ops, capsys, t0, decoupled, with_seed):
    n, k, stride = 1027, 3, 7919
    p, gr = _flat(n, 47 + t0, 2)
    steps = tuple(range(t0 + 1, t0 + k + 1))
    ref = _adam_oracle(decoupled, p, gr, steps, np.float64)

    def run():
        bp, bg = Buf(n, init=p, lead=LEAD), Buf(n, init=gr, lead=LEAD)
        bm, bv = Buf(n, init=np.zeros(1, np.float32), lead=LEAD), Buf(n, init=np.zeros(1, np.float32), lead=LEAD)
        bt = Buf(1, torch.int64, init=np.array([t0]))
        hyp = Buf(3, init=np.array([HP["lr"], np.nan, np.nan], np.float32))
        so = Buf(1, torch.int64) if with_seed else None
        for i in range(k):
            ops.step_begin(bt.v, hyp.v, so.v if with_seed else None, HP["b1"], HP["b2"], stride)
            step = t0 + i + 1
            assert bt.np()[0] == step
            if with_seed:
                assert so.np()[0] == (step - 1) * stride
            h = hyp.np()
            assert h[0] == HP["lr"]
            for j, b in ((1, HP["b1"]), (2, HP["b2"])):
                want = 1.0 - b ** step
                assert abs(h[j] - want) <= U * want, (step, j, h[j], want)   # f64 value, rounded once
            ops.adam_dev(bp.v, bg.v, bm.v, bv.v, n, hyp.v, HP["b1"], HP["b2"], HP["eps"], HP["wd"],
                         decoupled=decoupled)
        return bp, bm, bv, bt, hyp, so

    bp, bm, bv = twice(ops, run)[:3]
    _check_pmv(capsys, f"{'adamw' if decoupled else 'adam'}_dev t0={t0}", (bp.np(), bm.np(), bv.np()), ref,
               lambda: _adam_oracle(decoupled, p, gr, steps, np.float32))


@pytest.mark.parametrize("n", [1, 64, 65])
def test_counters_add_edges(ops, n):
    g = np.random.default_rng(n)
    size = n + 5
    arena0 = (1 << 40) + g.integers(0, 1 << 20, size)
    idx = g.permutation(size)[:n]
    val = (1 << 33) + g.integers(0, 1 << 20, n)
    want = arena0.copy()
    want[idx] += val
    ti, tv = dev(idx.astype(np.int64)), dev(val.astype(np.int64))

    def run():
        arena = Buf(size, torch.int64, init=arena0)
        ops.counters_add(arena.v, ti, tv)
        return (arena,)

    (arena,) = twice(ops, run)
    assert np.array_equal(arena.np(), want)


# ------------------------------------------------------------------------- small reductions
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 100003])
def test_sum_edges(ops, n):
    g = np.random.default_rng(n)
    x = (g.random(n, dtype=np.float32) + np.float32(0.25))       # positive: no cancellation
    scale = 0.37
    ref = x.astype(np.float64).sum() * f32(scale)
    tx = dev(x)

    def run():
        out = Buf(1)
        ops.sum_to(tx, n, scale, out.v)
        return (out,)

    (out,) = twice(ops, run)
    # f64 accumulation inside: the f64 value rounded once to f32
    assert abs(out.np()[0] - ref) <= 2 * U * abs(ref), (out.np()[0], ref)


@pytest.mark.parametrize("N", [1, 5, 4099])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 256])
def test_row_sqnorm_edges(ops, capsys, D, N):
    g = np.random.default_rng(100 * D + N)
    x = g.normal(size=(N, D)).astype(np.float32)
    if N >= 5:
        x[2] = 0.0
    ref = (x.astype(np.float64) ** 2).sum(axis=1)
    tx = dev(x)

    def run():
        out = Buf(N)
        ops.row_sqnorm(tx, N, D, out.v)
        return (out,)

    (out,) = twice(ops, run)
    # non-negative terms, <= 4 serial fmas + 6 tree additions per lane: <= 10 roundings of 2^-24
    err = np.abs(out.np() - ref) / np.where(ref > 0, ref, 1.0)
    within(capsys, f"row_sqnorm D={D} N={N}", err, 1e-6,
           lambda: np.abs((x * x).sum(axis=1) - ref) / np.where(ref > 0, ref, 1.0))


@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_bn_eval_coef_edges(ops, C):
    g = np.random.default_rng(C)
    gamma = (1 + g.uniform(-0.3, 0.3, C)).astype(np.float32)
    beta = g.uniform(-0.5, 0.5, C).astype(np.float32)
    rm = g.normal(size=C).astype(np.float32)
    rv = g.uniform(0.05, 4.0, C).astype(np.float32)
    eps = 1e-5
    sc = gamma.astype(np.float64) / np.sqrt(rv.astype(np.float64) + f32(eps))
    sh = beta.astype(np.float64) - rm.astype(np.float64) * sc
    ins = [dev(a) for a in (gamma, beta, rm, rv)]

    def run():
        scale, shift = Buf(C), Buf(C)
        ops.bn_eval_coef(*ins, scale.v, shift.v, eps=eps)
        return scale, shift

    scale, shift = twice(ops, run)
    # formed in f64 on the device and rounded once
    assert (np.abs(scale.np() - sc) <= 2 * U * np.abs(sc)).all()
    assert (np.abs(shift.np() - sh) <= 2 * U * np.abs(sh) + 1e-300).all()


# --------------------------------------------------------------------------------- kNN vote
@pytest.mark.parametrize("rerank", [False, True], ids=["gemm-rank", "rerank"])
@pytest.mark.parametrize("N", [5, 15, 16, 17, 255, 256, 257, 1000])
def test_knn_select_exact_ties(ops, N, rerank):
    """Integer features in [-4, 4], D = 24: every distance is an integer below 2^24, exact in
    f32 on both ranking paths, so the tie rules alone decide and O.knn_classify (stable argsort,
    smallest class) is the unique answer for every query."""
    M, D = 4, 24
    g = np.random.default_rng(N)
    X = g.integers(-4, 5, (N, D)).astype(np.float32)
    Q = g.integers(-4, 5, (M, D)).astype(np.float32)
    X[1] = X[N // 2] = X[N - 1]                       # three exact duplicates ...
    Q[0] = X[N - 1]                                   # ... at distance 0 from query 0
    ldS = N + 3
    S = np.full((M, ldS), np.float32(-1e9))           # padding: a read would be the nearest
    S[:, :N] = -2.0 * (Q @ X.T)
    xnorm = (X * X).sum(axis=1)
    d2 = xnorm[None] + S[:, :N] + (Q * Q).sum(axis=1)[:, None]
    assert d2.max() < 2 ** 24 and (d2 == np.round(d2)).all()
    assert any(len(np.unique(row)) < N for row in d2)                 # ties are present
    tS, tx, tQ, tX = dev(S), dev(xnorm), dev(Q), dev(X)
    for C in (1, 64):
        for K in (1, 5, 16):
            if K > N:
                continue
            lab = g.integers(0, C, N)
            _, nb = O.knn_classify(X, lab, Q, k=K)
            if C == 64 and K >= 4:                    # query 1: two classes tie, the smaller wins
                lab[nb[1]] = 63
                lab[nb[1][: 2 * (K // 2)]] = np.tile([50, 7], K // 2)
            pred_ref, nbr_ref = O.knn_classify(X, lab, Q, k=K)
            if C == 64 and K >= 4:
                assert pred_ref[1] == 7
            assert np.array_equal(nbr_ref[0][: min(K, 3)], [1, N // 2, N - 1][: min(K, 3)])
            tl = dev(lab.astype(np.int64))

            def run():
                nbr, pred, pred_only = Buf(M * K, torch.int64), Buf(M, torch.int64), Buf(M, torch.int64)
                kw = dict(Q=tQ, X=tX, D=D) if rerank else {}
                ops.knn_select(tS, ldS, tx, M, N, K, tl, C, nbr.v, pred.v, **kw)
                ops.knn_select(tS, ldS, tx, M, N, K, tl, C, None, pred_only.v, **kw)
                return nbr, pred, pred_only

            nbr, pred, pred_only = twice(ops, run)
            assert np.array_equal(nbr.np().reshape(M, K), nbr_ref), (C, K)
            assert np.array_equal(pred.np(), pred_ref) and np.array_equal(pred_only.np(), pred_ref), (C, K)


# ---------------------------------------------------------------------------------- staging
@pytest.mark.parametrize("HW", [4, 784, 12544])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G,L,orig", [(2, 4, True), (2, 0, True), (1, 3, False)])
def test_stage_views_edges(ops, G, L, orig, B, HW):
    g = np.random.default_rng(HW + 10 * B + G)
    gv = g.normal(size=(B, G, HW)).astype(np.float32)
    lv = g.normal(size=(B, L, HW)).astype(np.float32) if L else None
    ov = g.normal(size=(B, HW)).astype(np.float32) if orig else None
    pieces = [gv.transpose(1, 0, 2).reshape(-1, HW)]
    if L:
        pieces.append(lv.transpose(1, 0, 2).reshape(-1, HW))
    if orig:
        pieces.append(ov)
    ref = torch.from_numpy(np.concatenate(pieces).ravel())
    tg, tl, to = dev(gv), (dev(lv) if L else None), (dev(ov) if orig else None)

    def run():
        o32, o16 = Buf(ref.numel()), Buf(ref.numel(), torch.bfloat16)
        ops.stage_views(tg, G, tl, L, to, B, HW, o32.v)
        ops.stage_views(tg, G, tl, L, to, B, HW, o16.v)
        return o32, o16

    o32, o16 = twice(ops, run)
    assert same_bits(o32.v.cpu(), ref)
    assert same_bits(o16.v.cpu(), ref.to(torch.bfloat16))          # round to nearest even


# -------------------------------------------------------------------- dense activations
def _gelu_ref(x, dout, scale, shift, G):
    rows, C = x.shape
    z = x.reshape(G, rows // G, C) * scale.reshape(G, 1, C) + shift.reshape(G, 1, C)
    return O.gelu_fwd(z).reshape(rows, C), O.gelu_bwd(dout.reshape(z.shape), z).reshape(rows, C)


@pytest.mark.parametrize("rows,C", [(21, 5), (21, 300), (4098, 4096)],
                         ids=["21x5", "21x300", "second-grid-trip"])
def test_act_gelu_groups(ops, capsys, rows, C):
    """GELU over G = 3 groups of per-group scale / shift; 4098 x 4096 is just above the capped
    grid's 65536 x 256 threads."""
    G = 3
    g = np.random.default_rng(rows + C)
    x = g.standard_normal((rows, C), dtype=np.float32)
    dout = g.standard_normal((rows, C), dtype=np.float32)
    scale = (1 + g.uniform(-0.5, 0.5, (G, C))).astype(np.float32) * np.array([[0.5], [1.0], [2.0]], np.float32)
    shift = (g.uniform(-0.5, 0.5, (G, C)) + np.array([[-1.0], [0.0], [1.0]])).astype(np.float32)
    a_ref, dz_ref = _gelu_ref(x.astype(np.float64), dout.astype(np.float64), scale.astype(np.float64),
                              shift.astype(np.float64), G)
    tx, td, tsc, tsh = dev(x), dev(dout), dev(scale), dev(shift)

    def run():
        a, dz = Buf(rows * C), Buf(rows * C)
        ops.act_fwd(tx, a.v, 1, tsc, tsh, rows, G, C, 0.0, 0)
        ops.act_bwd(tx, td, dz.v, 1, tsc, tsh, rows, G, C, 0.0, 0)
        return a, dz

    a, dz = twice(ops, run)
    tag = f"gelu rows={rows} C={C}"
    within(capsys, tag + " fwd", row_rel(a.np(), a_ref), 1e-5,
           lambda: row_rel(_gelu_ref(x, dout, scale, shift, G)[0], a_ref))
    within(capsys, tag + " bwd", row_rel(dz.np(), dz_ref), 1e-5,
           lambda: row_rel(_gelu_ref(x, dout, scale, shift, G)[1], dz_ref))


def test_act_relu_exact_and_device_seed(ops):
    rows, C, G = 21, 300, 3
    g = np.random.default_rng(5)
    x = g.standard_normal((rows, C), dtype=np.float32)
    x[2, :7] = 0.0
    dout = g.standard_normal((rows, C), dtype=np.float32)
    scale = (1 + g.uniform(-0.5, 0.5, (G, C))).astype(np.float32)
    shift = g.uniform(-0.5, 0.5, (G, C)).astype(np.float32)
    tx, td, tsc, tsh = dev(x), dev(dout), dev(scale), dev(shift)
    k = 12345
    so = torch.tensor([k], dtype=torch.int64, device="cuda")

    def run():
        a, dx = Buf(rows * C), Buf(rows * C)
        ops.act_fwd(tx, a.v, 0, None, None, rows, 1, C, 0.0, 0)
        ops.act_bwd(tx, td, dx.v, 0, None, None, rows, 1, C, 0.0, 0)
        outs = [a, dx]
        for act, sc, sh, grp in ((0, None, None, 1), (1, tsc, tsh, G)):
            h_f, d_f, h_b, d_b = (Buf(rows * C) for _ in range(4))
            ops.act_fwd(tx, h_f.v, act, sc, sh, rows, grp, C, 0.3, 99 + k)
            ops.act_fwd(tx, d_f.v, act, sc, sh, rows, grp, C, 0.3, 99, so)
            ops.act_bwd(tx, td, h_b.v, act, sc, sh, rows, grp, C, 0.3, 99 + k)
            ops.act_bwd(tx, td, d_b.v, act, sc, sh, rows, grp, C, 0.3, 99, so)
            outs += [h_f, d_f, h_b, d_b]
        return outs

    outs = twice(ops, run)
    a, dx = outs[:2]
    assert np.array_equal(a.np(), np.maximum(x, 0).astype(np.float64).ravel())
    assert np.array_equal(dx.np(), np.where(x > 0, dout, 0).astype(np.float64).ravel())
    for i in (2, 6):
        h_f, d_f, h_b, d_b = outs[i:i + 4]
        assert same_bits(h_f.v, d_f.v) and same_bits(h_b.v, d_b.v)
    drop = float((outs[6].v == 0).float().mean())              # GELU is zero only where dropped
    assert 0.2 < drop < 0.4
