"""The ViT kernels (csrc/vit.hip) against float64 written out here: avd_mhsa_fwd / _bwd,
avd_ln_fwd / _bwd, avd_gelu_*, avd_vit_patchify, avd_vit_tokens_*.

Attention tiling named for the shapes below: a workgroup owns 16 rows of one (sequence, head) --
queries in the forward and the backward's row pass, keys in its column pass -- against all T keys
(queries), one per thread.  T = 197 = 12 * 16 + 5 is the audio ViT's own ragged case, T = 16 / 17
sit on and next to the tile edge, T = 50 is the image ViT's length, T = 1 / 5 are below one tile.
T = 256 = ops.MHSA_TMAX is the one length at which every thread holds a row and every 16-row tile
is full, 255 its ragged neighbour.  dh runs over ops.MHSA_HEAD_DIMS: each head size is its own
six kernels (forward, row pass, column pass, f32 and bf16).

LayerNorm: a lane holds elements l + 64 k; E = 96 leaves the middle chunk half valid, E = 480 the
last one; rows = 32800 is past the backward's 1024-block cap (trailing blocks own no row).  GELU:
8193 x 2048 elements is past 65536 blocks x 256 threads, so the grid-stride loop wraps.

f32 mode: rel-L2 < 1e-5 on ctx, lse, dQ, dK, dV (the band the engine's outputs take).
bf16 mode (computed, per output tensor, rel-L2): the same formulas in float64 with Q, K, V, dO
rounded to bf16, the dropped-out probabilities P o M rounded before P V and P^T dO, and dS rounded
before dS K and dS^T Q -- the kernel's roundings -- against unrounded float64, times 3.  The
measured error is printed beside the bound (run with -s).
"""
import math

import numpy as np
import pytest
import torch

from avdino import ops
from tests import vit_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 777.0
TILE = 16
MHSA_DHS = ops.MHSA_HEAD_DIMS                     # every dispatched head size
MHSA_TS = (1, 5, 16, 17, 50, 197, 255, 256)
MHSA_DROPOUT_CASES = [(3, 4, 17, 32, 0.1), (3, 4, 197, 32, 0.1), (3, 4, 197, 128, 0.5), (1, 1, 50, 128, 0.1),
                      (3, 4, 256, 64, 0.1)]
LN_ES = (32, 96, 480, 512)
LN_CAP_ROWS, LN_CAP_E = 32 * 1024 + 32, 32        # rows past the backward's block cap
GELU_WRAP = (8193, 2048)                          # 16 779 264 elements: just past 65536 x 256


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def rel(a, ref):
    return float((a - ref).norm() / ref.norm())


def make_inputs(N, heads, T, dh, seed, std=8.0):
    """f32 Q, K, V, dO [N, heads, T, dh]: logits scale Q K^T of std ~ ``std``, planted rows with
    |logit| > 100 whose maximum sits in the last / the first key tile, per-sequence V scales (and
    per-head offsets), as test_gpu_xattn.make_inputs."""
    g = torch.Generator().manual_seed(seed)
    scale = dh ** -0.5
    q = torch.randn(N, heads, T, dh, generator=g) * math.sqrt(std)
    k = torch.randn(N, heads, T, dh, generator=g) * math.sqrt(std)
    v = torch.randn(N, heads, T, dh, generator=g)
    do = torch.randn(N, heads, T, dh, generator=g)
    for n in range(N):
        v[n] *= 10.0 ** n                              # leakage between sequences shows at once
        for h in range(heads):
            v[n, h] += 3.0 * h                         # ... and between heads
            if T >= 2:
                for row, key, sign in ((0, T - 1, 1.0), (T - 1, 0, 1.0), (T // 2, T - 1, -1.0)):
                    kk = k[n, h, key]
                    q[n, h, row] = sign * kk * (120.0 / (scale * float(kk @ kk)))
    return q, k, v, do, scale


def mask_of(N, heads, T, p, seed):
    """The kernel's keep scale [N, heads, T, T] (float64), key ((n heads + h) T + i) T + j."""
    if p <= 0:
        return None
    idx = np.arange(N * heads * T * T, dtype=np.uint64)
    return torch.from_numpy(VR.dropout_scale(seed, idx, p).reshape(N, heads, T, T))


def reference(q, k, v, do, scale, mask, rounded):
    """float64 ctx, lse, dQ, dK, dV; rounded=True applies the kernel's bf16 roundings."""
    q, k, v, do = (t.to(torch.float64) for t in (q, k, v, do))
    m = 1.0 if mask is None else mask
    if rounded:
        q, k, v, do = bf(q), bf(k), bf(v), bf(do)
    s = scale * q @ k.transpose(-1, -2)
    p = s.softmax(-1)
    pd = p * m
    dp = (do @ v.transpose(-1, -2)) * m
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    if rounded:
        pd, ds = bf(pd), bf(ds)
    return (pd @ v, torch.logsumexp(s, -1), scale * ds @ k, scale * ds.transpose(-1, -2) @ q,
            pd.transpose(-1, -2) @ do)


def rows_of(t):
    """[N, heads, T, dh] -> the kernels' [N*T, heads*dh]."""
    N, heads, T, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(N * T, heads * dh)


def heads_of(t, N, heads, T, dh):
    return t.reshape(N, T, heads, dh).permute(0, 2, 1, 3)


def run_kernel(q, k, v, do, scale, bf16, p=0.0, seed=0, seed_off=None, with_lse=True):
    """Q / K / V as the column slices of a [rows + 1, 3E] buffer (one guard row), ctx and dctx as
    halves of [rows + 2, 2E] buffers, the gradients as slices of a [rows + 1, 4E] buffer; everything
    else sentinel."""
    N, heads, T, dh = q.shape
    E, rows = heads * dh, N * T
    qkv = torch.full((rows + 1, 3 * E), SENT)
    qkv[:rows] = torch.cat([rows_of(q), rows_of(k), rows_of(v)], -1)
    qkv = qkv.to(DEV)
    ob = torch.full((rows + 2, 2 * E), SENT, device=DEV)
    lse = torch.full((N * heads * T + 3,), SENT, device=DEV)
    ms = ((qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E))
    ops.mhsa_fwd(*ms, (ob, E, 2 * E), lse if with_lse else None, N, heads, T, dh, scale, bf16, p, seed, seed_off)
    if not with_lse:
        torch.cuda.synchronize()
        return ob.cpu(), None, None
    dob = torch.full((rows + 2, 2 * E), SENT)
    dob[:rows, :E] = rows_of(do)
    dob = dob.to(DEV)
    gb = torch.full((rows + 1, 4 * E), SENT, device=DEV)
    ws = torch.empty(ops.mhsa_bwd_ws(N, heads, T, dh), device=DEV)
    ops.mhsa_bwd((dob, 0, 2 * E), *ms, lse, (gb, 0, 4 * E), (gb, E, 4 * E), (gb, 3 * E, 4 * E), ws, N, heads, T,
                 dh, scale, bf16, p, seed, seed_off)
    torch.cuda.synchronize()
    return ob.cpu(), lse.cpu(), gb.cpu()


def check_case(N, heads, T, dh, bf16, p=0.0, seed=0, std=8.0):
    q, k, v, do, scale = make_inputs(N, heads, T, dh, 1000 * N + 100 * heads + 10 * T + dh, std)
    E, rows = heads * dh, N * T
    if T >= 2:
        s = scale * q.double() @ k.double().transpose(-1, -2)
        assert float(s.abs().max()) > 100.0 and 0.9 * std <= float(s.std())     # the inputs do their job
        if T > TILE:
            assert int(s[0, 0, 0].argmax()) >= (T - 1) // TILE * TILE and int(s[0, 0, T - 1].argmax()) < TILE
    mask = mask_of(N, heads, T, p, seed)
    exact = reference(q, k, v, do, scale, mask, rounded=False)
    model = reference(q, k, v, do, scale, mask, rounded=True)
    ob, lse, gb = run_kernel(q, k, v, do, scale, bf16, p, seed)
    ob2, lse2, gb2 = run_kernel(q, k, v, do, scale, bf16, p, seed)
    assert torch.equal(ob, ob2) and torch.equal(lse, lse2) and torch.equal(gb, gb2), "not bit-reproducible"
    ob3, _, _ = run_kernel(q, k, v, do, scale, bf16, p, seed, with_lse=False)
    assert torch.equal(ob, ob3), "a NULL lse changes ctx"
    # nothing outside the owned rows / columns is written
    assert bool((ob[:rows, :E] == SENT).all()) and bool((ob[rows:] == SENT).all())
    assert bool((lse[N * heads * T:] == SENT).all())
    assert bool((gb[rows:] == SENT).all()) and bool((gb[:rows, 2 * E:3 * E] == SENT).all())
    got = (heads_of(ob[:rows, E:], N, heads, T, dh), lse[:N * heads * T].reshape(N, heads, T),
           heads_of(gb[:rows, :E], N, heads, T, dh), heads_of(gb[:rows, E:2 * E], N, heads, T, dh),
           heads_of(gb[:rows, 3 * E:], N, heads, T, dh))
    for name, t, ex, mo in zip(("ctx", "lse", "dq", "dk", "dv"), got, exact, model):
        t = t.double()
        assert bool(torch.isfinite(t).all()), name
        tagline = f"mhsa N{N} h{heads} T{T} dh{dh} bf{int(bf16)} p{p} {name}"
        if float(ex.norm()) == 0.0:
            # T = 1: a one-key softmax has no gradient to its logit, dQ = dK = 0 exactly; the kernel
            # forms P (dP - delta) with delta = P dP / P from the same dP: zero up to one rounding
            dpm = float((do.double() * v.double()).sum(-1).abs().max())
            lim = 1e-6 * scale * dpm * float(max(q.abs().max(), k.abs().max()))
            print(f"{tagline}: max |.| {float(t.abs().max()):.2e} (limit {lim:.2e})")
            assert float(t.abs().max()) <= lim, name
            continue
        err = rel(t, ex)
        bound = 3.0 * rel(mo, ex) if bf16 else 1e-5
        print(f"{tagline}: rel-L2 {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (name, err, bound)
    return mask


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("dh", MHSA_DHS)
@pytest.mark.parametrize("T", MHSA_TS)
@pytest.mark.parametrize("N,heads", [(1, 1), (3, 1), (1, 4), (3, 4)])
def test_mhsa_matches_float64(N, heads, T, dh, bf16):
    check_case(N, heads, T, dh, bf16)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N,heads,T,dh,p", MHSA_DROPOUT_CASES)
def test_mhsa_dropout_matches_float64_with_the_numpy_mask(N, heads, T, dh, p, bf16):
    mask = check_case(N, heads, T, dh, bf16, p=p, seed=(1 << 50) + 977)
    if mask.numel() >= 131072:
        kept = float((mask > 0).double().mean())
        print(f"kept fraction {kept:.4f} of {mask.numel()} (1 - p = {1 - p})")
        assert abs(kept - (1 - p)) < 0.01


def test_mhsa_milder_logits_and_the_device_seed_offset():
    """Logits of std ~ 1 (no planted rows dominate the tensor norms less); and seed + *seed_off
    equals the seed passed directly."""
    check_case(2, 4, 50, 32, False, std=1.0)
    check_case(2, 4, 50, 32, True, std=1.0)
    q, k, v, do, scale = make_inputs(2, 2, 17, 32, 5)
    off = torch.tensor([48], dtype=torch.int64, device=DEV)
    a = run_kernel(q, k, v, do, scale, False, 0.1, 1000, off)
    b = run_kernel(q, k, v, do, scale, False, 0.1, 1048)
    c = run_kernel(q, k, v, do, scale, False, 0.1, 1000)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])


def test_mhsa_rejects_bad_shapes_and_strides_without_a_launch():
    N, heads, T, dh = 2, 2, 5, 32
    E, R = heads * dh, N * T
    qkv = torch.full((R, 3 * E), SENT, device=DEV)
    ctx = torch.full((R, E), SENT, device=DEV)
    ms = ((qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E))
    with pytest.raises(ValueError):
        ops.mhsa_fwd(*ms, (ctx, 0, E), None, N, heads, 300, dh, 0.1, False)
    with pytest.raises(ValueError):
        ops.mhsa_fwd(*ms, (ctx, 0, E), None, N, 1, T, 48, 0.1, False)
    from avdino._lib import lib
    a = qkv.data_ptr()
    args = lambda q=a, ld=3 * E, T=T, dh=dh: (q, ld, a + 4 * E, ld, a + 8 * E, ld, ctx.data_ptr(), E, None,  # noqa: E731
                                             N, heads, T, dh, 0, 0.1, 0.0, 0, None, None)
    assert lib.avd_mhsa_fwd(*args(T=257)) == -1 and lib.avd_mhsa_fwd(*args(dh=48)) == -1
    assert lib.avd_mhsa_fwd(*args(q=a + 4)) == -4 and lib.avd_mhsa_fwd(*args(ld=3 * E + 2)) == -4
    torch.cuda.synchronize()
    assert bool((ctx == SENT).all())                 # nothing ran


# ---------------------------------------------------------------- LayerNorm
def ln_reference(x, r, mask, gamma, beta, dy, eps=1e-5):
    x, gamma, beta, dy = (t.double() for t in (x, gamma, beta, dy))
    x = x.clone().requires_grad_(True)
    gamma, beta = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = x
    if r is not None:
        r = r.double().clone().requires_grad_(True)
        z = x + r * (1.0 if mask is None else mask)
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    y = (z - mu) / torch.sqrt(var + eps) * gamma + beta
    y.backward(dy)
    return y.detach(), x.grad, None if r is None else r.grad, gamma.grad, beta.grad


def check_layer_norm(rows, E, with_r, pad, p, poison_ws=False):
    """ln_fwd / ln_bwd against float64: y, dx, dr, dgamma, dbeta, the pad columns, the constant
    row, bit-reproducibility.  poison_ws: the backward's workspace is all NaN before each call, so
    a block that skips its partial write shows in dgamma and dbeta."""
    g = torch.Generator().manual_seed(rows * 1000 + E + pad)
    x = torch.randn(rows, E, generator=g) * 2.0 + 0.5
    r = torch.randn(rows, E, generator=g) if with_r else None
    const = rows // 2 if rows > 1 else None          # one row of constant values: variance 0
    if const is not None:                            # (alone it would make dgamma exactly zero)
        x[const] = 1.25
        if with_r:
            r[const] = 0.0
    gamma = 1.0 + 0.2 * torch.randn(E, generator=g)
    beta = 0.2 * torch.randn(E, generator=g)
    dy = torch.randn(rows, E, generator=g)
    seed = 4242
    mask = None
    if p > 0:
        mask = torch.from_numpy(VR.dropout_scale(seed, np.arange(rows * E, dtype=np.uint64), p).reshape(rows, E))
    ry, rdx, rdr, rdg, rdb = ln_reference(x, r, mask, gamma, beta, dy)
    ld = E + pad

    def strided(t):
        b = torch.full((rows, ld), SENT)
        b[:, :E] = t
        return b.to(DEV)

    xd, dyd = strided(x), strided(dy)
    rd = strided(r) if with_r else None
    yd = torch.full((rows, ld), SENT, device=DEV)
    z, mean, rstd = (torch.empty(n, device=DEV) for n in (rows * E, rows, rows))
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ops.ln_fwd(xd, rd, gd, bd, yd, rows, E, z, mean, rstd, 1e-5, p, seed, None, x_ld=ld, res_ld=ld, y_ld=ld)
    y2 = torch.full((rows, ld), SENT, device=DEV)
    ops.ln_fwd(xd, rd, gd, bd, y2, rows, E, None, None, None, 1e-5, p, seed, None, x_ld=ld, res_ld=ld, y_ld=ld)
    assert torch.equal(yd, y2)                       # the saved state changes nothing
    dx = torch.full((rows, ld), SENT, device=DEV)
    dr = torch.full((rows, ld), SENT, device=DEV) if with_r else None
    ws = torch.empty(ops.ln_bwd_ws(rows, E), device=DEV)
    runs = []
    for _ in range(2):
        dg, db = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
        if poison_ws:
            ws.fill_(float("nan"))
        ops.ln_bwd(dyd, z, mean, rstd, gd, dx, dr, dg, db, ws, rows, E, p, seed, None, dy_ld=ld, dx_ld=ld, dr_ld=ld)
        runs.append((dx.cpu().clone(), dg.cpu(), db.cpu()) + ((dr.cpu().clone(),) if with_r else ()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "layer norm gradients not bit-reproducible"
    yh = yd.cpu()
    if pad:
        assert bool((yh[:, E:] == SENT).all()) and bool((runs[0][0][:, E:] == SENT).all())
    if const is not None:
        assert float(rstd[const]) == pytest.approx(1e-5 ** -0.5, rel=1e-5)
        assert rel(yh[const, :E].double(), beta.double()) < 1e-6
    errs = dict(y=rel(yh[:, :E].double(), ry), dx=rel(runs[0][0][:, :E].double(), rdx),
                dgamma=rel(runs[0][1].double(), rdg), dbeta=rel(runs[0][2].double(), rdb))
    if with_r:
        errs["dr"] = rel(runs[0][3][:, :E].double(), rdr)
    print(f"ln rows{rows} E{E} r{int(with_r)} pad{pad} p{p}:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < (1e-5 if k in ("dgamma", "dbeta") else 1e-6), (k, v)


@pytest.mark.parametrize("with_r,pad,p", [(False, 0, 0.0), (True, 0, 0.0), (True, 24, 0.0), (False, 24, 0.0),
                                          (True, 0, 0.1), (True, 24, 0.1)])     # dropout: on the branch
@pytest.mark.parametrize("E", LN_ES)
@pytest.mark.parametrize("rows", [1, 7, 300])
def test_layer_norm_matches_float64(rows, E, with_r, pad, p):
    check_layer_norm(rows, E, with_r, pad, p)


@pytest.mark.parametrize("with_r,p", [(False, 0.0), (True, 0.1)])
def test_layer_norm_past_the_backward_block_cap(with_r, p):
    """More than 32 x 1024 rows: the backward's grid is capped, a block walks rpb = 33 rows and
    the blocks from 994 on own none -- they must still write zero partials."""
    rows, E = LN_CAP_ROWS, LN_CAP_E
    blocks = ops.ln_bwd_ws(rows, E) // (2 * E)
    rpb = -(-rows // blocks)
    assert blocks == 1024 and rpb == 33 and 993 * rpb < rows <= 994 * rpb
    check_layer_norm(rows, E, with_r, 0, p, poison_ws=True)


def test_final_norm_on_the_cls_rows_with_a_token_stride():
    """The tower's last LayerNorm: rows T*E apart in, dense out; the backward writes the cls rows of
    a [N, T, E] gradient and nothing else."""
    N, T, E = 3, 5, 64
    g = torch.Generator().manual_seed(3)
    h = torch.randn(N, T, E, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(E, generator=g), 0.2 * torch.randn(E, generator=g)
    dy = torch.randn(N, E, generator=g)
    ry, rdx, _, rdg, rdb = ln_reference(h[:, 0], None, None, gamma, beta, dy)
    hd, y = h.reshape(-1).to(DEV), torch.empty(N * E, device=DEV)
    z, mean, rstd = (torch.empty(n, device=DEV) for n in (N * E, N, N))
    ops.ln_fwd(hd, None, gamma.to(DEV), beta.to(DEV), y, N, E, z, mean, rstd, x_ld=T * E)
    dh = torch.full((N, T, E), SENT, device=DEV)
    dg, db = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
    ws = torch.empty(ops.ln_bwd_ws(N, E), device=DEV)
    ops.ln_bwd(dy.to(DEV), z, mean, rstd, gamma.to(DEV), dh.view(-1), None, dg, db, ws, N, E, dx_ld=T * E)
    assert rel(y.cpu().double().view(N, E), ry) < 1e-6
    assert rel(dh[:, 0].cpu().double(), rdx) < 1e-6 and bool((dh[:, 1:] == SENT).all())
    assert rel(dg.cpu().double(), rdg) < 1e-5 and rel(db.cpu().double(), rdb) < 1e-5


# ---------------------------------------------------------------- GELU, patches, tokens
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows,C", [(1, 1), (7, 33), (300, 2048)])
def test_gelu_matches_float64(rows, C, p):
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) * 2.0
    do = torch.randn(rows, C, generator=g)
    seed = 99
    m = torch.from_numpy(VR.dropout_scale(seed, np.arange(rows * C, dtype=np.uint64), p).reshape(rows, C))
    x64 = x.double().requires_grad_(True)
    out = 0.5 * x64 * (1.0 + torch.erf(x64 / math.sqrt(2.0))) * m
    out.backward(do.double())
    xd, o, dx = x.to(DEV), torch.empty(rows * C + 1, device=DEV), torch.empty(rows * C + 1, device=DEV)
    o[-1], dx[-1] = SENT, SENT
    ops.gelu_fwd(xd, o, rows, C, p, seed)
    ops.gelu_bwd(xd, do.to(DEV), dx, rows, C, p, seed)
    assert float(o[-1]) == SENT and float(dx[-1]) == SENT
    eo, ed = rel(o[:-1].cpu().double().view(rows, C), out.detach()), rel(dx[:-1].cpu().double().view(rows, C), x64.grad)
    print(f"gelu {rows}x{C} p{p}: out {eo:.2e} dx {ed:.2e}")
    assert eo < 1e-6 and ed < 1e-6
    if p > 0 and rows * C >= 131072:
        assert abs(float((m > 0).double().mean()) - (1 - p)) < 0.01
        oh = o[:-1].cpu().view(rows, C)
        assert bool((oh[m == 0] == 0).all()) and bool((oh[(m > 0) & (x.abs() > 1e-3) & (x.abs() < 4)] != 0).all())


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_past_the_grid_cap(p):
    """More elements than 65536 blocks x 256 threads: the grid-stride loop takes a second trip for
    the elements from 16 777 216 on (the audio ViT's MLP activation is there from N = 42)."""
    rows, C = GELU_WRAP
    n, wrap = rows * C, 65536 * 256
    assert n > wrap
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(n, generator=g) * 2.0
    do = torch.randn(n, generator=g)
    seed = 99
    m = torch.from_numpy(VR.dropout_scale(seed, np.arange(n, dtype=np.uint64), p))
    x64 = x.double()
    cdf = 0.5 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))
    out = x64 * cdf * m
    dx64 = do.double() * m * (cdf + x64 * torch.exp(-0.5 * x64 * x64) / math.sqrt(2.0 * math.pi))
    xd, o, dx = x.to(DEV), torch.empty(n + 1, device=DEV), torch.empty(n + 1, device=DEV)
    o[-1], dx[-1] = SENT, SENT
    ops.gelu_fwd(xd, o, rows, C, p, seed)
    ops.gelu_bwd(xd, do.to(DEV), dx, rows, C, p, seed)
    assert float(o[-1]) == SENT and float(dx[-1]) == SENT
    oh, dh = o[:-1].cpu(), dx[:-1].cpu()
    eo, ed = rel(oh.double(), out), rel(dh.double(), dx64)
    ew, edw = rel(oh[wrap:].double(), out[wrap:]), rel(dh[wrap:].double(), dx64[wrap:])
    print(f"gelu {rows}x{C} p{p}: out {eo:.2e} dx {ed:.2e}; wrapped part out {ew:.2e} dx {edw:.2e}")
    assert eo < 1e-6 and ed < 1e-6 and ew < 1e-6 and edw < 1e-6
    if p > 0:
        mw, xw = m[wrap:], x[wrap:]
        assert 0 < int((mw == 0).sum()) < mw.numel()
        assert bool((oh[wrap:][mw == 0] == 0).all()) and bool((dh[wrap:][mw == 0] == 0).all())
        assert bool((oh[wrap:][(mw > 0) & (xw.abs() > 1e-3) & (xw.abs() < 4)] != 0).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,H,P", [(1, 16, 8), (3, 16, 8), (1, 112, 8), (3, 112, 8)])
def test_patchify_is_exact(N, H, P, dt):
    g = torch.Generator().manual_seed(N + H)
    x = torch.rand(N, 1, H, H, generator=g).to(dt)
    want = VR.patch_rows(x.float(), P).reshape(-1, P * P)
    # the conv weight's (ph, pw) order: one GEMM row per patch equals Conv2d(1, E, P, stride P)
    w = torch.randn(4, 1, P, P, generator=g)
    conv = torch.nn.functional.conv2d(x.double(), w.double(), stride=P).flatten(2).transpose(1, 2).reshape(-1, 4)
    assert rel(want.double() @ w.double().reshape(4, -1).T, conv) < 1e-12
    out = torch.full((N * H * H + 1,), SENT, device=DEV)
    ops.vit_patchify(x.reshape(-1).to(DEV), out, N, H, H, P)
    assert float(out[-1]) == SENT
    assert torch.equal(out[:-1].cpu().view(-1, P * P), want)


@pytest.mark.parametrize("N,T,E", [(1, 5, 32), (3, 5, 32), (3, 197, 512)])
def test_tokens_forward_and_backward(N, T, E):
    g = torch.Generator().manual_seed(N + T)
    pe, cls, pos = torch.randn(N, T - 1, E, generator=g), torch.randn(E, generator=g), torch.randn(T, E, generator=g)
    want = torch.cat([cls.expand(N, 1, E), pe], 1) + pos
    tok = torch.full((N * T * E + 1,), SENT, device=DEV)
    ops.vit_tokens_fwd(pe.reshape(-1).to(DEV), cls.to(DEV), pos.reshape(-1).to(DEV), tok, N, T, E)
    assert float(tok[-1]) == SENT and torch.equal(tok[:-1].cpu().view(N, T, E), want)    # one f32 add each
    dtok = torch.randn(N, T, E, generator=g)
    dpe = torch.full((N * (T - 1) * E + 1,), SENT, device=DEV)
    dd = dtok.reshape(-1).to(DEV)
    ops.vit_tokens_bwd(dd, dpe, N, T, E)
    assert float(dpe[-1]) == SENT and torch.equal(dpe[:-1].cpu().view(N, T - 1, E), dtok[:, 1:])
    dpos = torch.empty(T * E, device=DEV)
    ops.sum_rows(dd, N, T * E, dpos)
    assert rel(dpos.cpu().double().view(T, E), dtok.double().sum(0)) < 1e-6
