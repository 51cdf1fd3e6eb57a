"""SimCLR view augmentation on the GPU: the elastic and blur stages of avd_augment_views_x against
the float64 restatement (tests/simclr_aug_ref.py), the old kinds through the new export bit for
bit, the device parameter draws, and AVMNISTSimCLRDataModule feeding a SimCLR training run.

Tolerance of the pixel tests: the same restatement evaluated in float32 NumPy on the test's own
inputs deviates from its float64 result by ``d32``; the kernel is allowed ``TOL_FACTOR * d32``.
The factor covers the kernel's own rounding choices inside that float32 budget (device expf, the
summation order of the taps).  Measured on these inputs (every test prints its own), d32 and, in
brackets, the kernel's deviation on an MI355X:
  blur K=3: 28x28 1.81e-07 (2.02e-07), 16x20 1.86e-07 (1.86e-07), 112x112 2.28e-07 (2.28e-07)
  blur K=5: 28x28 2.10e-07 (2.18e-07), 16x20 1.99e-07 (2.40e-07), 112x112 2.51e-07 (3.46e-07)
  elastic:  28x28 sigma 3 7.30e-07 (7.30e-07), 16x20 sigma 1.5 1.09e-06 (1.09e-06),
            14x16 sigma 3.3 1.46e-06 (1.35e-06);   full image chain 5.97e-07 (5.97e-07)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from avdino import augment as A  # noqa: E402
from avdino import ops  # noqa: E402
from oracle import augment as OA  # noqa: E402

from . import simclr_aug_ref as R  # noqa: E402
from .test_augment_data import _fake_avmnist  # noqa: E402
from .test_gpu_augment import _records, _stats  # noqa: E402

TOL_FACTOR = 4.0
SEED = 0xDEADBEEF12345


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_x(src, idx, lut, rec, ext, V, H, W, kinds, order=0, dtype=torch.float32, gm=None, seed=SEED):
    B = len(idx)
    out = torch.empty((B, V, H, W) if order == 0 else (V, B, H, W), device="cuda", dtype=dtype)
    ops.augment_views_x(_cuda(src), _cuda(np.asarray(idx, np.int64)), _cuda(lut), _cuda(rec),
                        None if gm is None else _cuda(gm.view(np.int32)), 4, seed, V, H, W, out, order,
                        kinds, None if ext is None else _cuda(ext))
    return out


def _blank_records(n):
    rec = np.zeros((n, A.REC), np.float32)
    rec[:, 22] = -1
    return rec


def _case(H, W, seed, N=5, B=4, V=2):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (N, H * W), dtype=np.uint8)
    idx = rng.integers(0, N, B)
    lut = OA.normalise_lut("image")
    imgs = lut[src[idx]].reshape(B, H, W)
    return src, idx, lut, imgs, B, V


def _check(got, ref64, ref32, what):
    d32 = np.abs(ref32.astype(np.float64) - ref64).max()
    err = np.abs(got.astype(np.float64) - ref64).max()
    print(f"{what}: float32 restatement deviates {d32:.3e}, kernel {err:.3e}, "
          f"allowed {TOL_FACTOR * d32:.3e}")
    assert np.isfinite(got).all()
    assert d32 > 0
    assert err <= TOL_FACTOR * d32, (what, err, d32)


# --------------------------------------------------------------- old kinds, new export
@pytest.mark.parametrize("mod", ["image", "audio"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_old_kind_chains_are_bit_identical_through_the_x_export(mod, order, dtype):
    H = W = 28 if mod == "image" else 112
    N, B, V = 11, 5, 2
    rng = np.random.default_rng(31)
    src = rng.integers(0, 256, (N, H * W), dtype=np.uint8)
    idx = rng.integers(0, N, B)
    lut = OA.normalise_lut(mod)
    chain = A.default_chains()["local"][mod]      # image: 4 stages; audio: 7, noise and groups too
    rec, gm = _records([(k, kw, 1.0) for k, kw, _p in chain], B, V, H, W, 5)
    kinds = A.chain_kinds(chain)
    ref = torch.empty((B, V, H, W) if order == 0 else (V, B, H, W), device="cuda", dtype=dtype)
    ops.augment_views(_cuda(src), _cuda(idx), _cuda(lut), _cuda(rec),
                      None if gm is None else _cuda(gm.view(np.int32)), 4, SEED, V, H, W, ref, order,
                      kinds)
    got = _run_x(src, idx, lut, rec, None, V, H, W, kinds, order, dtype, gm)
    assert torch.equal(got, ref)
    assert torch.isfinite(ref.float()).all() and (ref != 0).any()
    # an ext of zeros (both stages off) and the new kinds in the chain (the elastic one where the
    # map is small enough for it): still the same views
    ext = np.zeros((B * V, A.XREC), np.float32)
    new = [R.K_ELASTIC, R.K_BLUR] if H * W <= 1024 else [R.K_BLUR]
    got = _run_x(src, idx, lut, rec, ext, V, H, W, kinds[:2] + new + kinds[2:], order, dtype, gm)
    assert torch.equal(got, ref)


# ---------------------------------------------------------------------- single stages
@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("H,W", [(28, 28), (16, 20), (112, 112)])
def test_blur_stage_matches_the_restatement(H, W, K):
    src, idx, lut, imgs, B, V = _case(H, W, 100 + K)
    rec = _blank_records(B * V)
    ext = np.zeros((B * V, A.XREC), np.float32)
    ext[:, R.X_SIGMA] = np.linspace(0.1, 1.2, B * V)      # every record on
    ext[:, R.X_K] = K
    got = _run_x(src, idx, lut, rec, ext, V, H, W, [R.K_BLUR]).cpu().numpy()
    ref = {dt: np.stack([R.blur(imgs[r // V], ext[r, 0], K, dt) for r in range(B * V)])
           for dt in (np.float64, np.float32)}
    assert np.abs(ref[np.float64] - imgs.repeat(V, 0)).max() > 0.1     # the stage did something
    _check(got.reshape(B * V, H, W), ref[np.float64], ref[np.float32], f"blur K={K} {H}x{W}")


@pytest.mark.parametrize("H,W,sigma", [(28, 28, 3.0), (16, 20, 1.5), (14, 16, 3.3)])
def test_elastic_stage_matches_the_restatement(H, W, sigma):
    """14 x 16 with sigma 3.3: K_e = 27, radius 13 = H - 1, the reflect limit."""
    src, idx, lut, imgs, B, V = _case(H, W, 200 + H)
    rec = _blank_records(B * V)
    ext = np.zeros((B * V, A.XREC), np.float32)
    ext[:, R.X_ALPHA], ext[:, R.X_ESIGMA] = 20.0, sigma
    assert R.elastic_taps(sigma) // 2 <= min(H, W) - 1
    got = _run_x(src, idx, lut, rec, ext, V, H, W, [R.K_ELASTIC]).cpu().numpy()
    ref = {}
    outside = 0
    for dt in (np.float64, np.float32):
        o = []
        for r in range(B * V):
            nx, ny = R.noise_fields(SEED, r, H, W)
            info = {}
            o.append(R.elastic(imgs[r // V], 20.0, sigma, nx, ny, dt, info))
            outside += int(((info["ix"] < 0) | (info["ix"] > W - 1) | (info["iy"] < 0) |
                            (info["iy"] > H - 1)).sum())
        ref[dt] = np.stack(o)
    assert outside > 0                                                 # the mask term is exercised
    assert np.abs(ref[np.float64] - imgs.repeat(V, 0)).max() > 0.1
    _check(got.reshape(B * V, H, W), ref[np.float64], ref[np.float32], f"elastic {H}x{W}")


@pytest.mark.parametrize("H,W", [(28, 28), (16, 20)])
def test_elastic_noise_fields_are_the_numpy_hash_bit_for_bit(H, W):
    """No export hands out the noise fields, so they are pinned through the pixels: with a sigma
    whose Gaussian has one tap (K_e = int(8 * 0.01 + 1) = 1, weight exactly 1) the smoothed field
    IS the noise field, and everything after it is +, -, *, floor -- no transcendental -- so the
    float32 restatement in the kernel's operation order reproduces the kernel's output bit for
    bit if and only if it starts from the same noise bits.  The second half shows the check has
    that resolution: one mantissa step (2^-23) on either field changes most output pixels (those
    it cannot change sample outside the map or between equal neighbours; alpha = 8 keeps the
    unsmoothed displacements, up to alpha / 2 pixels, mostly inside)."""
    src, idx, lut, imgs, B, V = _case(H, W, 300 + H)
    rec = _blank_records(B * V)
    ext = np.zeros((B * V, A.XREC), np.float32)
    alpha = 8.0
    ext[:, R.X_ALPHA], ext[:, R.X_ESIGMA] = alpha, 0.01
    assert R.elastic_taps(0.01) == 1
    got = _run_x(src, idx, lut, rec, ext, V, H, W, [R.K_ELASTIC]).cpu().numpy().reshape(B * V, H, W)
    step = np.float32(2.0 ** -23)
    changed = []
    for r in range(B * V):
        nx, ny = R.noise_fields(SEED, r, H, W)
        want = R.elastic(imgs[r // V], alpha, 0.01, nx, ny, np.float32)
        assert want.dtype == np.float32
        np.testing.assert_array_equal(got[r], want)
        for fx, fy in ((nx + step, ny), (nx, ny + step)):
            changed.append((R.elastic(imgs[r // V], alpha, 0.01, fx, fy, np.float32) != want).mean())
    print(f"share of pixels one noise ulp changes: min {min(changed):.3f}")
    assert min(changed) > 0.5
    assert np.abs(got - imgs.repeat(V, 0)).max() > 0.1


# ------------------------------------------------------------------------ the full image chain
def test_default_image_chain_matches_the_restatement():
    """simclr_chains()['image'] with host records; records cycle through neither / elastic / blur
    / both.  Records with neither stage are bit-exact against oracle.augment.augment_one_seq."""
    H = W = 28
    N, B, V = 11, 6, 2
    rng = np.random.default_rng(41)
    src = rng.integers(0, 256, (N, H * W), dtype=np.uint8)
    idx = rng.integers(0, N, B)
    lut = OA.normalise_lut("image")
    chain = A.simclr_chains()["image"]
    aug = A.ViewAugmenter.__new__(A.ViewAugmenter)
    aug.rng, aug.H, aug.W = np.random.default_rng(9), H, W
    rec, gm, ext = aug.records([(k, kw, 1.0) for k, kw, _p in chain], B, V)
    assert gm is None and (ext[:, 0] > 0).all() and (ext[:, 2] == 20).all()
    n = B * V
    mode = np.arange(n) % 4
    ext[(mode == 0) | (mode == 2), 2:] = 0          # elastic off
    ext[(mode == 0) | (mode == 1), :2] = 0          # blur off
    ext[2, 0] = 0.45                                # one blur-only record with a sigma that shows
    kinds = A.chain_kinds(chain)
    assert kinds == [0, 4, 5, 9, 10]
    got = _run_x(src, idx, lut, rec, ext, V, H, W, kinds).cpu().numpy().reshape(n, H, W)
    imgs = lut[src[idx]].reshape(B, H, W)
    ref = {dt: np.stack([R.augment_one_x(imgs[r // V], rec[r], ext[r], None, SEED, r, kinds, dt=dt)
                         for r in range(n)]) for dt in (np.float64, np.float32)}
    plain = np.stack([OA.augment_one_seq(imgs[r // V], rec[r], None, SEED, r, kinds) for r in range(n)])
    off = mode == 0
    np.testing.assert_array_equal(got[off], plain[off])
    # the new stages did something (a blur with sigma near 0.1 is the identity to rounding)
    moved = np.abs(ref[np.float64] - plain).reshape(n, -1).max(1)
    assert (moved[(mode == 1) | (mode == 3)] > 1e-3).all() and moved[2] > 1e-3 and (moved[off] == 0).all()
    _check(got[~off], ref[np.float64][~off], ref[np.float32][~off], "image chain")


# ----------------------------------------------------------------------------- device draws
def test_device_draws_of_the_new_kinds():
    n, H, W = 4096, 28, 28
    chain = A.simclr_chains()["image"]
    aug = A.ViewAugmenter(torch.zeros(1, H * W, dtype=torch.uint8, device="cuda"),
                          torch.zeros(256, device="cuda"), H, W, seed=77)
    rec, gm, ext = aug.records_dev(chain, n, 1)
    rec, ext = rec.cpu().numpy(), ext.cpu().numpy()
    assert gm is None and ext.shape == (n, A.XREC)
    band = 5 * np.sqrt(0.3 * 0.7 / n)
    ela, blr = ext[:, 2] != 0, ext[:, 0] > 0
    print(f"applied shares: elastic {ela.mean():.4f}, blur {blr.mean():.4f} (band {band:.4f})")
    assert abs(ela.mean() - 0.3) < band and abs(blr.mean() - 0.3) < band
    assert (ext[ela, 2] == 20).all() and (ext[ela, 3] == 3).all() and (ext[~ela, 2:] == 0).all()
    assert (ext[blr, 1] == 3).all() and (ext[~blr, :2] == 0).all()
    sg = ext[blr, 0]
    assert sg.min() >= 0.1 and sg.max() <= 0.5
    assert abs(sg.mean() - 0.3) < 5 * (0.4 / np.sqrt(12)) / np.sqrt(blr.sum())
    assert abs((ela & blr).mean() - 0.09) < 5 * np.sqrt(0.09 * 0.91 / n)
    # the old fields: the bands of test_gpu_augment's device-draw test, against the host sampler
    hrec, _hgm, _hext = aug.records(chain, 20000, 1)
    ds, hs = _stats(rec, None, H, W), _stats(hrec, None, H, W)
    assert ds.keys() == hs.keys()
    for k in ds:
        if k.startswith("p_"):
            assert abs(ds[k] - hs[k]) < 0.015, (k, ds[k], hs[k])
        else:
            assert abs(ds[k] - hs[k]) <= 0.03 * max(abs(hs[k]), 1e-3) + 0.002, (k, ds[k], hs[k])
    # deterministic in the seed; the views run from device records
    aug2 = A.ViewAugmenter(aug.src, aug.lut, H, W, seed=77)
    rec2, _, ext2 = aug2.records_dev(chain, n, 1)
    assert np.array_equal(rec2.cpu().numpy(), rec) and np.array_equal(ext2.cpu().numpy(), ext)


# ------------------------------------------------------------------------------- end to end
class _Labelled:
    """(image, audio, label) loaders over the fake files, as train_and_evaluate_ssl needs them."""

    def __init__(self, root):
        self.root = root

    def setup(self, stage=None):
        from avdino.data import AVMNISTLabelledLoader
        mk = lambda split: AVMNISTLabelledLoader(self.root, batch_size=16, split=split,  # noqa: E731
                                                 train_size=36, val_size=4, seed=3)
        self.tr, self.va, self.te = mk("train"), mk("val"), mk("test")

    def train_dataloader(self):
        return self.tr

    def val_dataloader(self):
        return self.va

    def test_dataloader(self):
        return self.te


def test_data_module_feeds_a_simclr_run(tmp_path, monkeypatch):
    from avdino import training_structures as T
    from avdino.data import AVMNISTSimCLRDataModule
    from avdino.models import MultiModalSimCLRLightning
    data = tmp_path / "data"
    data.mkdir()
    root = _fake_avmnist(data, n=40)
    dm = AVMNISTSimCLRDataModule(root, batch_size=8, train_size=36, val_size=4, seed=3)
    dm.setup()
    train = dm.train_dataloader()
    assert len(train) == 5 and len(dm.val_dataloader()) == 1
    batches = list(train)
    assert [b[0].shape[0] for b in batches] == [8, 8, 8, 8, 4]
    i1, a1, i2, a2 = batches[0]
    assert i1.shape == i2.shape == (8, 1, 28, 28) and a1.shape == a2.shape == (8, 1, 112, 112)
    for t in (i1, a1, i2, a2):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
        assert torch.isfinite(t).all()
    for b in range(8):                          # two independent views of every sample
        assert not torch.equal(i1[b], i2[b]) and not torch.equal(a1[b], a2[b])
    first = [b[0].clone() for b in train]        # the next epoch reshuffles and redraws
    assert not torch.equal(first[0], i1)
    (v1, _, _, _), = list(dm.val_dataloader())
    assert v1.shape == (4, 1, 28, 28)
    img, aud, lab = next(iter(dm.test_dataloader()))
    assert img.shape == (8, 1, 28, 28) and aud.shape == (8, 1, 112, 112) and lab.shape == (8,)

    module = MultiModalSimCLRLightning(projection_dim=16, output_dim=32, use_mixed_precision=False,
                                       num_epochs=1, device="cuda", seed=4)
    loss = module.training_step(batches[0], 0, mode=2)
    assert np.isfinite(loss.item())

    monkeypatch.chdir(tmp_path)            # the summary is written to the working directory
    perf = T.train_and_evaluate_ssl(module, dm, _Labelled(root), str(tmp_path / "run"), "simclr_aug",
                                    seeds=[1], num_epochs=1)
    lines = (tmp_path / "simclr_aug_performance_summary.txt").read_text().splitlines()
    assert lines[0].startswith("model_name") and len(lines) == 9
    assert (tmp_path / "run" / "simclr_aug_seed1.ckpt").is_file()
    assert set(perf["per_seed"]) == {"image", "audio"}
