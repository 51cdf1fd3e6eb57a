"""Host side of the SimCLR view augmentation (no GPU, nothing here launches a kernel): the blur /
elastic restatement (tests/simclr_aug_ref.py) pinned to torch's own ops composed the way
torchvision composes them, the chains and host parameter draws, and the argument checks of the
two ``_x`` exports."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from avdino import augment as A
from avdino import ops

from . import simclr_aug_ref as R

SHAPE, ARG = -1, -4        # AVD_ERR_SHAPE, AVD_ERR_ARG (include/avdino.h)


# ------------------------------------------------------------------ restatement vs torch ops
def _torch_blur(img, sigma, K):
    """torchvision gaussian_blur: reflect pad K//2, conv2d with outer(w, w), float64."""
    x = torch.linspace(-(K - 1) * 0.5, (K - 1) * 0.5, K, dtype=torch.float64)
    w = torch.exp(-0.5 * (x / sigma) ** 2)
    w = w / w.sum()
    k2 = torch.outer(w, w)[None, None]
    t = torch.from_numpy(np.asarray(img, np.float64))[None, None]
    t = F.pad(t, [K // 2] * 4, mode="reflect")
    return F.conv2d(t, k2)[0, 0].numpy()


def _torch_elastic(img, alpha, sigma, nx, ny):
    """ElasticTransform.get_params on given noise + elastic_transform (bilinear, fill 0)."""
    H, W = img.shape
    K = R.elastic_taps(sigma)
    # get_params: dx = blur(noise) * alpha / size[0], dy = blur(noise) * alpha / size[1]
    dx = torch.from_numpy(_torch_blur(nx, float(sigma), K)) * alpha / H
    dy = torch.from_numpy(_torch_blur(ny, float(sigma), K)) * alpha / W
    # _create_identity_grid([H, W]) + displacement, then grid_sample on img with a ones channel
    gx = torch.linspace((-W + 1) / W, (W - 1) / W, W, dtype=torch.float64)
    gy = torch.linspace((-H + 1) / H, (H - 1) / H, H, dtype=torch.float64)
    grid = torch.stack([gx[None, :].expand(H, W) + dx, gy[:, None].expand(H, W) + dy], -1)[None]
    t = torch.from_numpy(np.asarray(img, np.float64))
    t = torch.stack([t, torch.ones_like(t)])[None]
    o = F.grid_sample(t, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]
    return (o[0] * o[1] + (1.0 - o[1]) * 0.0).numpy()      # img * mask + (1 - mask) * fill


@pytest.mark.parametrize("H,W,sigma", [(28, 28, 3.0), (16, 20, 1.5)])
def test_restatement_matches_torch_ops(H, W, sigma):
    rng = np.random.default_rng(H * W)
    img = rng.random((H, W))
    for K, s in ((3, 0.1), (3, 0.5), (5, 0.8), (7, 1.3)):
        np.testing.assert_allclose(R.blur(img, s, K), _torch_blur(img, s, K), rtol=0, atol=1e-12)
    nx, ny = rng.random((H, W)) * 2 - 1, rng.random((H, W)) * 2 - 1
    info = {}
    got = R.elastic(img, 20.0, sigma, nx, ny, info=info)
    ix, iy = info["ix"], info["iy"]
    outside = (ix < 0) | (ix > W - 1) | (iy < 0) | (iy > H - 1)
    assert outside.any(), "no displaced sample outside the map: the mask term is not exercised"
    np.testing.assert_allclose(got, _torch_elastic(img, 20.0, sigma, nx, ny), rtol=0, atol=1e-12)
    # the smoothing alone (rows then columns) against torch's outer-product kernel
    K = R.elastic_taps(sigma)
    np.testing.assert_allclose(R.smooth(nx, sigma), _torch_blur(nx, sigma, K), rtol=0, atol=1e-12)


def test_elastic_taps_and_hash_fields():
    assert [R.elastic_taps(s) for s in (3.0, 1.5, 3.3, 0.01)] == [25, 13, 27, 1]
    assert [A.elastic_taps(s) for s in (3.0, 1.5, 3.3, 0.01)] == [25, 13, 27, 1]
    nx, ny = R.noise_fields(0xDEADBEEF12345, 7, 14, 16)
    assert nx.dtype == np.float32 and nx.shape == (14, 16)
    for f in (nx, ny):
        assert f.min() >= -1 and f.max() < 1 and abs(f.mean()) < 0.2
    assert not np.array_equal(nx, ny)
    assert not np.array_equal(nx, R.noise_fields(0xDEADBEEF12345, 8, 14, 16)[0])


# ------------------------------------------------------------------------- chains and draws
def test_simclr_chains_are_the_reference_defaults():
    ch = A.simclr_chains()
    assert ch["image"] == [
        ("crop", dict(scale=(0.5, 1.0), ratio=(0.8, 1.2)), 1.0),
        ("rotation", dict(degrees=5), 1.0),
        ("affine", dict(translate=(0.1, 0.1)), 1.0),
        ("elastic", dict(alpha=20.0, sigma=3.0), 0.3),
        ("blur", dict(kernel_size=3, sigma=(0.1, 0.5)), 0.3)]
    assert ch["audio"] == [
        ("crop", dict(scale=(0.5, 1.0)), 1.0),
        ("time_warp", dict(min_factor=0.9, max_factor=1.1), 0.5),
        ("frequency_mask", dict(freq_mask_param=10), 0.5),
        ("time_mask", dict(time_mask_param=10), 0.5),
        ("gaussian_noise", dict(std=0.05), 0.3)]
    assert A.chain_kinds(ch["image"]) == [0, 4, 5, 9, 10]
    assert not A.fixed_order(ch["image"]) and A.fixed_order(ch["audio"])
    assert not A.fixed_order([("blur", dict(kernel_size=3, sigma=(0.1, 0.5)), 1.0)])
    assert not A.fixed_order([("elastic", dict(alpha=20.0, sigma=3.0), 1.0)])
    st = A.chain_stages(ch["image"], H=28, W=28)
    assert st.shape == (5, 8)
    assert st[3].tolist() == [9, np.float32(0.3), 20, 3, 0, 0, 0, 0]
    assert st[4].tolist() == [10, np.float32(0.3), 3, np.float32(0.1), 0.5, 0, 0, 0]


def test_chain_validation_of_the_new_kinds():
    ok = [("elastic", dict(alpha=20.0, sigma=3.0), 0.3), ("blur", dict(kernel_size=5, sigma=(0.1, 0.5)), 1.0)]
    A.validate_chain(ok)
    A.validate_chain(ok, 28, 28)
    for K in (1, 4, 9):
        with pytest.raises(ValueError):
            A.validate_chain([("blur", dict(kernel_size=K, sigma=(0.1, 0.5)), 1.0)])
    with pytest.raises(ValueError):
        A.validate_chain([("blur", dict(kernel_size=3, sigma=(0.5, 0.1)), 1.0)])
    with pytest.raises(ValueError):       # H*W > 1024
        A.validate_chain(ok[:1], 34, 34)
    with pytest.raises(ValueError):       # K_e/2 = 13 > min(H, W) - 1 = 11
        A.validate_chain([("elastic", dict(alpha=20.0, sigma=3.3), 1.0)], 12, 16)
    A.validate_chain([("elastic", dict(alpha=20.0, sigma=3.3), 1.0)], 14, 16)
    with pytest.raises(NotImplementedError):
        A.validate_chain(ok + ok[:1])
    for bare in (("elastic", dict(alpha=20.0), 1.0), ("blur", dict(kernel_size=3), 1.0)):
        with pytest.raises(NotImplementedError):  # parameters are spelled out, never defaulted
            A.validate_chain([bare])
    with pytest.raises(NotImplementedError):     # the 2-tuple sampler has no room for ext
        A.sample_records(np.random.default_rng(0), ok, 4, 28, 28)


def test_host_draw_statistics():
    n = 4096
    chain = A.simclr_chains()["image"]
    rec, gm, ext = A.sample_records_x(np.random.default_rng(11), chain, n, 28, 28)
    assert rec.shape == (n, A.REC) and ext.shape == (n, A.XREC) and gm is None
    band = 5 * np.sqrt(0.3 * 0.7 / n)
    ela, blr = ext[:, 2] != 0, ext[:, 0] > 0
    assert abs(ela.mean() - 0.3) < band and abs(blr.mean() - 0.3) < band
    assert (ext[ela, 2] == 20).all() and (ext[ela, 3] == 3).all() and (ext[~ela, 2:] == 0).all()
    assert (ext[blr, 1] == 3).all() and (ext[~blr, :2] == 0).all()
    sg = ext[blr, 0]
    assert sg.min() >= 0.1 and sg.max() <= 0.5
    assert abs(sg.mean() - 0.3) < 5 * (0.4 / np.sqrt(12)) / np.sqrt(blr.sum())
    assert abs((ela & blr).mean() - 0.09) < 5 * np.sqrt(0.09 * 0.91 / n)    # independent draws
    # the old stages of the chain are drawn as before
    assert (rec[:, 23] == 7).all() and (rec[:, 2] > 0).all()
    # ViewAugmenter.records: (rec, gm, ext) for a chain with the new kinds, (rec, gm) otherwise
    aug = A.ViewAugmenter.__new__(A.ViewAugmenter)
    aug.rng, aug.H, aug.W = np.random.default_rng(2), 28, 28
    r3 = aug.records(chain, 6, 2)
    assert len(r3) == 3 and r3[0].shape == (12, A.REC) and r3[2].shape == (12, A.XREC)
    assert len(aug.records(A.default_chains()["local"]["image"], 6, 2)) == 2


# -------------------------------------------------------------- argument checks, no launch
def _stages(*rows):
    st = np.zeros((len(rows), 8), np.float32)
    for i, r in enumerate(rows):
        st[i, :len(r)] = r
    return st


def test_argument_validation_without_launch():
    from avdino._lib import lib
    d = ctypes.c_void_p(16)

    def views(kinds, H, W, ext=d):
        ks = np.asarray(kinds, np.int32)
        return lib.avd_augment_views_x(d, d, 4, 2, 1, H, W, d, d, None, 0, 4, 1, 0, ks.ctypes.data,
                                       len(kinds), d, 0, ext, None)

    def records(st, H, W, ext=d):
        return lib.avd_augment_records_x(st.ctypes.data, st.shape[0], 8, H, W, 4, 1, d, None, 0,
                                         ext, None)

    assert views([9], 34, 34) == SHAPE                       # elastic with H*W = 1156 > 1024
    assert records(_stages([9, 1, 20, 3]), 34, 34) == SHAPE
    assert records(_stages([9, 1, 20, 3.3]), 12, 16) == SHAPE     # K_e/2 = 13 > min(H, W) - 1 = 11
    assert records(_stages([9, 1, 20, 3]), 12, 20) == SHAPE       # K_e/2 = 12 > 11
    for K in (4, 1, 9, 2, 8, 3.5):                                # blur K even or outside 3..7
        assert records(_stages([10, 1, K, 0.1, 0.5]), 28, 28) == SHAPE, K
    assert records(_stages([10, 1, 7, 0.1, 0.5]), 2, 8) == SHAPE  # K/2 = 3 > min(H, W) - 1 = 1
    assert views([0] * 12, 28, 28) == SHAPE                       # 12 stages
    assert records(_stages(*[[2, 1, 5]] * 12), 28, 28) == SHAPE
    assert views([11], 28, 28) == ARG and views([-1], 28, 28) == ARG
    assert views([0, 10], 28, 28, ext=None) == ARG                # new kind, no ext
    assert views([9], 28, 28, ext=None) == ARG
    assert records(_stages([10, 1, 3, 0.1, 0.5]), 28, 28, ext=None) == ARG
    assert records(_stages([9, 1, 20, 3]), 28, 28, ext=None) == ARG
    # the old exports keep their limits: 9 stages, kinds 0..8
    ks = np.asarray([9], np.int32)
    assert lib.avd_augment_views_seq(d, d, 4, 2, 1, 28, 28, d, d, None, 0, 4, 1, 0, ks.ctypes.data, 1,
                                     d, 0, None) == ARG
    ks = np.zeros(10, np.int32)
    assert lib.avd_augment_views_seq(d, d, 4, 2, 1, 28, 28, d, d, None, 0, 4, 1, 0, ks.ctypes.data, 10,
                                     d, 0, None) == SHAPE


def test_ops_argument_checks():
    B, V, H, W = 2, 2, 28, 28
    src = torch.zeros(3, H * W, dtype=torch.uint8)
    idx = torch.zeros(B, dtype=torch.int64)
    lut = torch.zeros(256)
    rec = torch.zeros(B * V, ops.AUG_REC)
    out = torch.zeros(B * V * H * W)
    ext = torch.zeros(B * V, ops.AUG_XREC)
    args = (src, idx, lut, rec, None, 4, 0, V, H, W, out, 0)
    with pytest.raises(ValueError, match="ext dtype"):
        ops.augment_views_x(*args, [10], ext.double())
    with pytest.raises(ValueError, match="ext numel"):
        ops.augment_views_x(*args, [10], ext[:3])
    with pytest.raises(ValueError, match="ext missing"):
        ops.augment_views_x(*args, [9], None)
    with pytest.raises(ValueError, match="stage kinds"):
        ops.augment_views_x(*args, [0] * 12, ext)
    H2 = W2 = 34
    with pytest.raises(ValueError, match="1024"):
        ops.augment_views_x(torch.zeros(3, H2 * W2, dtype=torch.uint8), idx, lut, rec, None, 4, 0, V,
                            H2, W2, torch.zeros(B * V * H2 * W2), 0, [9], ext)
    st = _stages([9, 1, 20, 3])
    with pytest.raises(ValueError, match="ext dtype"):
        ops.augment_records_x(st, 4, H, W, 4, 0, rec, None, ext.double())
    with pytest.raises(ValueError, match="ext numel"):
        ops.augment_records_x(st, 4, H, W, 4, 0, rec, None, ext[:3])
    with pytest.raises(ValueError, match="1024"):
        ops.augment_records_x(st, 4, H2, W2, 4, 0, rec, None, ext)
    with pytest.raises(ValueError, match="aug stages"):
        ops.augment_records_x(_stages(*[[2, 1, 5]] * 12), 4, H, W, 4, 0, rec, None, ext)


# ------------------------------------------------------------------------ the augmentation class
def test_simclr_augmentation_keeps_the_default_chains_with_augment_values():
    """The reference builds an audio chain from augment_values and never uses it
    (get_data.py:371-390): the default transforms stay."""
    av = {"augmentations": {"time_warp": {"min_factor": 0.5, "max_factor": 1.5},
                            "gaussian_noise": {"std": 0.3}},
          "augmentation_probabilities": {"time_warp": 1.0, "gaussian_noise": 1.0}}
    aug = A.SimCLRMultiModalAugmentation(augment_values=av)
    ch = A.simclr_chains()
    assert aug.image_transform == ch["image"] and aug.spectrogram_transform == ch["audio"]
    assert A.SimCLRMultiModalAugmentation().image_transform == ch["image"]
    with pytest.raises(KeyError):
        A.SimCLRMultiModalAugmentation(augment_values={
            "augmentations": {"random_resized_crop": {}}, "augmentation_probabilities": {}})
    with pytest.raises(KeyError):         # a probability is needed per name, as in the reference
        A.SimCLRMultiModalAugmentation(augment_values={
            "augmentations": {"time_mask": {"time_mask_param": 5}}, "augmentation_probabilities": {}})
    for kw in (dict(image_size=32), dict(spec_size=96)):
        with pytest.raises(NotImplementedError):
            A.SimCLRMultiModalAugmentation(**kw)
    assert aug.bind("i", "a") is aug and (aug.image, aug.audio) == ("i", "a")


def test_data_module_signature_and_exports():
    import inspect

    from avdino import data as D
    assert D.SimCLRMultiModalAugmentation is A.SimCLRMultiModalAugmentation
    sig = inspect.signature(D.AVMNISTSimCLRDataModule.__init__)
    assert list(sig.parameters) == ["self", "data_dir", "batch_size", "num_workers", "type",
                                    "augmentations", "device", "seed", "train_size", "val_size"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["batch_size"], d["num_workers"], d["type"], d["train_size"], d["val_size"]) == (
        128, 6, "burst_noise", 55000, 5000)
    dm = D.AVMNISTSimCLRDataModule("/nowhere/")
    assert isinstance(dm.augmentations, A.SimCLRMultiModalAugmentation)
    with pytest.raises(FileNotFoundError):
        dm.setup()
