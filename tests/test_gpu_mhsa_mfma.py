"""avd_mhsa_mfma_fwd / _bwd (csrc/mhsa_mfma.hip), the bf16 tensor-core attention of the ViT tower,
against float64: ctx, lse, dQ, dK, dV.  Inputs, mask and the float64 formulas are those of
tests/test_gpu_vit_ops.py (imported), the operands sit in its strided, sentinel-guarded layout.

Tiling named for the shapes: a wave owns 16 query rows (key rows in the column pass), a workgroup
4 waves = 64 rows, the other side streams in 32-row blocks.  T = 16 / 17 sit on and past the wave,
31 / 32 / 33 around the streamed block, 63 / 64 / 65 around the workgroup (at 65 the second
workgroup has one row in wave 0 and none in waves 1-3, which must still stage and meet every
barrier), 1 / 5 are below one wave, 50 and 197 the towers' own lengths, 255 / 256 the limit
ops.MHSA_TMAX.  (N, heads) = (3, 4) puts every (sequence, head) offset in play.

Band, per tensor: rel-L2 <= 3 x rel(reference(rounded=True), reference(rounded=False)), the
project's rounding-model band of the bf16 mode.  The kernel's own roundings differ in place
(flash form: the unnormalised masked exp(s - m) is rounded, the f32 accumulator divided by the
row sum at the end; delta is formed relative to the top-P key); an f32 emulation of exactly that
form on these inputs stays at or below 0.35 of the band on every tensor.  The measured error is
printed beside the bound (run with -s).
"""
import pytest
import torch

from avdino import ops
from tests.test_gpu_vit_ops import (DEV, MHSA_DROPOUT_CASES, SENT, heads_of, make_inputs, mask_of, reference, rel,
                                    rows_of)

pytestmark = pytest.mark.gpu

MFMA_TS = (1, 5, 16, 17, 31, 32, 33, 50, 63, 64, 65, 197, 255, 256)
MFMA_DROPOUT_CASES = MHSA_DROPOUT_CASES + [(2, 2, 65, 64, 0.1)]


def run_kernel(q, k, v, do, scale, p=0.0, seed=0, seed_off=None, with_lse=True):
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
    ops.mhsa_mfma_fwd(*ms, (ob, E, 2 * E), lse if with_lse else None, N, heads, T, dh, scale, p, seed, seed_off)
    if not with_lse:
        torch.cuda.synchronize()
        return ob.cpu(), None, None
    dob = torch.full((rows + 2, 2 * E), SENT)
    dob[:rows, :E] = rows_of(do)
    dob = dob.to(DEV)
    gb = torch.full((rows + 1, 4 * E), SENT, device=DEV)
    ws = torch.empty(ops.mhsa_mfma_bwd_ws(N, heads, T, dh), device=DEV)
    ops.mhsa_mfma_bwd((dob, 0, 2 * E), *ms, lse, (gb, 0, 4 * E), (gb, E, 4 * E), (gb, 3 * E, 4 * E), ws, N, heads,
                      T, dh, scale, p, seed, seed_off)
    torch.cuda.synchronize()
    return ob.cpu(), lse.cpu(), gb.cpu()


def check_case(N, heads, T, dh, p=0.0, seed=0):
    q, k, v, do, scale = make_inputs(N, heads, T, dh, 1000 * N + 100 * heads + 10 * T + dh)
    E, rows = heads * dh, N * T
    mask = mask_of(N, heads, T, p, seed)
    exact = reference(q, k, v, do, scale, mask, rounded=False)
    model = reference(q, k, v, do, scale, mask, rounded=True)
    ob, lse, gb = run_kernel(q, k, v, do, scale, p, seed)
    ob2, lse2, gb2 = run_kernel(q, k, v, do, scale, p, seed)
    assert torch.equal(ob, ob2) and torch.equal(lse, lse2) and torch.equal(gb, gb2), "not bit-reproducible"
    ob3, _, _ = run_kernel(q, k, v, do, scale, p, seed, with_lse=False)
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
        tagline = f"mhsa_mfma N{N} h{heads} T{T} dh{dh} p{p} {name}"
        if float(ex.norm()) == 0.0:
            # T = 1: dQ = dK = 0 exactly; the absolute limit of test_gpu_vit_ops.check_case
            dpm = float((do.double() * v.double()).sum(-1).abs().max())
            lim = 1e-6 * scale * dpm * float(max(q.abs().max(), k.abs().max()))
            print(f"{tagline}: max |.| {float(t.abs().max()):.2e} (limit {lim:.2e})")
            assert float(t.abs().max()) <= lim, name
            continue
        err, bound = rel(t, ex), 3.0 * rel(mo, ex)
        print(f"{tagline}: rel-L2 {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (name, err, bound)
    return mask


@pytest.mark.parametrize("dh", ops.MHSA_HEAD_DIMS)
@pytest.mark.parametrize("T", MFMA_TS)
@pytest.mark.parametrize("N,heads", [(1, 1), (3, 4)])
def test_mhsa_mfma_matches_float64(N, heads, T, dh):
    check_case(N, heads, T, dh)


@pytest.mark.parametrize("N,heads,T,dh,p", MFMA_DROPOUT_CASES)
def test_mhsa_mfma_dropout_matches_float64_with_the_numpy_mask(N, heads, T, dh, p):
    """The mask is the numpy restatement of the hash: a wrong key, or a mask applied to the row sum,
    is an O(1) error on every tensor."""
    mask = check_case(N, heads, T, dh, p=p, seed=(1 << 50) + 977)
    if mask.numel() >= 131072:
        kept = float((mask > 0).double().mean())
        print(f"kept fraction {kept:.4f} of {mask.numel()} (1 - p = {1 - p})")
        assert abs(kept - (1 - p)) < 0.01


def test_mhsa_mfma_device_seed_offset_equals_the_seed_passed_directly():
    q, k, v, do, scale = make_inputs(2, 2, 17, 32, 5)
    off = torch.tensor([48], dtype=torch.int64, device=DEV)
    a = run_kernel(q, k, v, do, scale, 0.1, 1000, off)
    b = run_kernel(q, k, v, do, scale, 0.1, 1048)
    c = run_kernel(q, k, v, do, scale, 0.1, 1000)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])


def test_mhsa_mfma_rejects_bad_shapes_and_strides_without_a_launch():
    N, heads, T, dh = 2, 2, 5, 32
    E, R = heads * dh, N * T
    qkv = torch.full((R, 3 * E), SENT, device=DEV)
    ctx = torch.full((R, E), SENT, device=DEV)
    dqkv = torch.full((R, 3 * E), SENT, device=DEV)
    lse = torch.zeros(N * heads * T, device=DEV)
    ws = torch.full((N * heads * T,), SENT, device=DEV)
    ms = ((qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E))
    with pytest.raises(ValueError):
        ops.mhsa_mfma_fwd(*ms, (ctx, 0, E), None, N, heads, 300, dh, 0.1)
    with pytest.raises(ValueError):
        ops.mhsa_mfma_fwd(*ms, (ctx, 0, E), None, N, 1, T, 48, 0.1)
    from avdino._lib import lib
    a, g = qkv.data_ptr(), dqkv.data_ptr()

    def fwd(q=a, ld=3 * E, T=T, dh=dh):
        return lib.avd_mhsa_mfma_fwd(q, ld, a + 4 * E, ld, a + 8 * E, ld, ctx.data_ptr(), E, None, N, heads, T, dh,
                                     0.1, 0.0, 0, None, None)

    def bwd(q=a, ld=3 * E, T=T, dh=dh, n_ws=ws.numel()):
        return lib.avd_mhsa_mfma_bwd(ctx.data_ptr(), E, q, ld, a + 4 * E, ld, a + 8 * E, ld, lse.data_ptr(),
                                     g, 3 * E, g + 4 * E, 3 * E, g + 8 * E, 3 * E, ws.data_ptr(), n_ws,
                                     N, heads, T, dh, 0.1, 0.0, 0, None, None)

    assert fwd(T=257) == -1 and fwd(T=0) == -1 and fwd(dh=48) == -1
    assert fwd(q=a + 4) == -4 and fwd(ld=3 * E + 2) == -4 and fwd(ld=E - 4) == -4
    assert bwd(T=257) == -1 and bwd(dh=48) == -1
    assert bwd(q=a + 4) == -4 and bwd(ld=3 * E + 2) == -4 and bwd(n_ws=ws.numel() - 1) == -4
    torch.cuda.synchronize()
    assert bool((ctx == SENT).all()) and bool((dqkv == SENT).all()) and bool((ws == SENT).all())   # nothing ran
