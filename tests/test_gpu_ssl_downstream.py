"""Downstream evaluation of a trained SimCLR model's towers and their late fusion
(``is_dino_based=False``) against the reference's own results, and the experiment driver.

Fixtures ssl_downstream_{image,audio,fusion}[_f64] (tests/golden/gen_ssl_golden.py): the
reference's train_knn_classifier / train_downstream / compute_classification_metrics on its
MultiModalSimCLRModel's image_encoder, audio_encoder and a concat LateFusionEncoder, run on CPU in
float32 and float64 (D = 32, batch 16, 3 / 2 / 2 batches, 2 epochs).  The generator asserts that
the two precisions agree on every kNN prediction, validation accuracy and test prediction.

Bands (f32 engine vs the float64 fixture).  The image tower is the network of
test_gpu_downstream.py's image_simple case and takes its constants: features rel-L2 1e-5,
per-epoch losses 1e-4 abs, classifier rel 1e-4; decisions identical, kNN neighbour sets under
that file's tie rule (contested distances equal within 1e-5 relative).  Audio and fusion allow
the larger of those constants and 4x the reference's own |f32 - f64| difference stored in the
fixture (4x: the engine's f32 MFMA sums in another order than torch's CPU conv).  The stored
differences are 2.0e-7 .. 2.3e-7 (features), 1.1e-7 .. 2.7e-7 (losses) and 0.9e-7 .. 1.7e-7
(classifier), so 4x stays below the constants and the resulting bands are 1e-5 / 1e-4 / 1e-4
for all three targets."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import spec as S  # noqa: E402
from oracle.params import make_multimodal_batch, make_simclr_batch, make_state  # noqa: E402
from tests import golden_util as gu  # noqa: E402

FEAT, LOSS, CLS, MARGIN = 1e-5, 1e-4, 1e-4, 4.0     # test_gpu_downstream.py's constants


def _loader(B, n, seed):
    out = []
    for i in range(n):
        b = make_multimodal_batch(B, 1, 0, seed + i)
        out.append(tuple(torch.from_numpy(b[k]).cuda() for k in ("image", "audio", "label")))
    return out


def _target(model, target):
    from avdino.training_structures import LateFusionEncoder
    if target == "fusion":
        return LateFusionEncoder(model.audio_encoder, model.image_encoder, fusion="concat")
    return getattr(model, f"{target}_encoder")


@pytest.mark.parametrize("target", ["image", "audio", "fusion"])
def test_ssl_downstream_matches_reference(target, tmp_path):
    from avdino import downstream as DS
    from avdino.models import MultiModalSimCLRModel
    fx64 = gu.load(f"ssl_downstream_{target}_f64")
    D, P, B, nt, nv, ne, epochs, pseed, bseed = [int(x) for x in fx64["meta_dims"]]
    lr = float(fx64["meta_lr"])
    assert str(fx64["meta_target"]) == target
    band = {"feat": FEAT, "loss": LOSS, "cls": CLS}
    if target != "image":
        band = {"feat": max(FEAT, MARGIN * max(float(fx64["refdiff/feat_train"]), float(fx64["refdiff/feat_test"]))),
                "loss": max(LOSS, MARGIN * float(fx64["refdiff/history"])),
                "cls": max(CLS, MARGIN * float(fx64["refdiff/cls"]))}
    print(f"{target}: bands {band}")
    model = MultiModalSimCLRModel(output_dim=D, projection_dim=P, device="cuda", precision="32")
    state = make_state(S.simclr_spec(D, P), pseed)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    enc = _target(model, target)
    tr, va, te = _loader(B, nt, bseed), _loader(B, nv, bseed + 1000), _loader(B, ne, bseed + 2000)
    # frozen eval-mode features
    fe = DS.FeatureExtractor(enc, is_dino_based=False)
    assert fe.output_dim == (2 * D if target == "fusion" else D)
    assert fe.modality == (None if target == "fusion" else target)
    trf, _ = DS.feature_extraction_loop("cuda", fe, tr)
    tef, _ = DS.feature_extraction_loop("cuda", fe, te)
    for key, val in (("feat_train", trf), ("feat_test", tef)):
        ok, msg = gu.compare(fx64, key, val.cpu().numpy(), rel=band["feat"])
        print(msg)
        assert ok, msg
    # kNN: the reference's predictions exactly; neighbours up to f32-equidistant ties
    knn, acc = DS.train_knn_classifier(enc, tr, te, n_neighbors=5, is_dino_based=False)
    np.testing.assert_array_equal(knn.predict(tef).cpu().numpy(), fx64["knn_pred"])
    nb, rnb = knn.kneighbors(tef).cpu().numpy(), fx64["knn_nbr"]
    qf, xf = np.asarray(fx64["feat_test"], np.float64), np.asarray(fx64["feat_train"], np.float64)
    d64 = ((qf[:, None, :] - xf[None]) ** 2).sum(-1)
    for i in np.nonzero((nb != rnb).any(1))[0]:
        assert set(nb[i]) == set(rnb[i]), i
        dd = np.take(d64[i], nb[i])
        j = np.nonzero(nb[i] != rnb[i])[0]
        assert np.ptp(dd[j]) <= 1e-5 * dd[j].max(), (i, dd)
    assert acc == pytest.approx(float(fx64["knn_acc"]))
    # the MLP probe: AdamW + cosine LR, best-val checkpoint, test evaluation
    cls = {k: torch.from_numpy(np.array(v))
           for k, v in make_state(S.classifier_spec(fe.output_dim), pseed + 1).items()}
    clf = DS.train_downstream(enc, tr, va, te, num_epochs=epochs, learning_rate=lr,
                              save_path=str(tmp_path / "d" / "m.pt"),
                              train_log_path=str(tmp_path / "d" / "train.csv"),
                              test_log_path=str(tmp_path / "d" / "test.csv"), is_dino_based=False,
                              classifier_state=cls)
    hist = np.array([[h["train_loss"], h["val_loss"], h["val_accuracy"]] for h in clf.history])
    print("history |diff|", np.abs(hist[:, :2] - fx64["history"][:, :2]).max())
    np.testing.assert_allclose(hist[:, :2], fx64["history"][:, :2], atol=band["loss"], rtol=0)
    np.testing.assert_array_equal(hist[:, 2], fx64["history"][:, 2])
    met = DS.compute_classification_metrics(clf, te)
    np.testing.assert_array_equal(met["predictions"], fx64["test_preds"])
    assert met["accuracy"] == pytest.approx(float(fx64["test_acc"]))
    np.testing.assert_array_equal(met["confusion_matrix"], fx64["confusion_matrix"])
    for k, v in clf.classifier_state_dict().items():
        ok, msg = gu.compare(fx64, "cls/" + k, v.cpu().numpy(), rel=band["cls"])
        assert ok, msg
    # the trained model itself was never touched (frozen deep copy)
    for k, v in state.items():
        assert np.allclose(model.store[k].detach().cpu().numpy(), v), k


@pytest.mark.parametrize("fusion", ["sum", "mean"])
def test_late_fusion_sum_mean_features(fusion):
    """sum / mean fusion = the two towers' own features added (halved), bit for bit."""
    from avdino import downstream as DS
    from avdino.models import MultiModalSimCLRModel
    from avdino.training_structures import LateFusionEncoder
    model = MultiModalSimCLRModel(output_dim=32, projection_dim=16, device="cuda", precision="32", seed=5)
    (img, aud, _lab), = _loader(5, 1, 77)
    zi = DS.FeatureExtractor(model.image_encoder, is_dino_based=False)(img, aud)
    za = DS.FeatureExtractor(model.audio_encoder, is_dino_based=False)(img, aud)
    z = DS.FeatureExtractor(LateFusionEncoder(model.audio_encoder, model.image_encoder, fusion=fusion),
                            is_dino_based=False)(img, aud)
    ref = zi + za if fusion == "sum" else (zi + za) / 2
    assert torch.equal(z, ref)


class _TestData:
    """(image, audio, label) loaders of two batches of 16, as the drivers need them."""

    def __init__(self):
        self.ready = False

    def setup(self, stage=None):
        self.ready = True
        self.tr, self.va, self.te = _loader(16, 2, 500), _loader(16, 2, 1500), _loader(16, 2, 2500)

    def train_dataloader(self):
        return self.tr

    def val_dataloader(self):
        return self.va

    def test_dataloader(self):
        return self.te


def test_train_and_evaluate_ssl_end_to_end(tmp_path, monkeypatch):
    from avdino import training_structures as T
    from avdino.models import MultiModalSimCLRLightning
    monkeypatch.chdir(tmp_path)            # the summaries are written to the working directory
    module = MultiModalSimCLRLightning(projection_dim=16, output_dim=32, use_mixed_precision=False,
                                       num_epochs=1, device="cuda", seed=4)
    train = []
    for i in range(2):
        b = make_simclr_batch(16, 900 + i)
        train.append(tuple(torch.from_numpy(b[k]).cuda() for k in ("img1", "spec1", "img2", "spec2")))
    data = _TestData()
    model_dir = str(tmp_path / "run")
    perf = T.train_and_evaluate_ssl(module, train, data, model_dir, "simclr", seeds=[1, 2], num_epochs=1)
    assert data.ready
    lines = (tmp_path / "simclr_performance_summary.txt").read_text().splitlines()
    assert [ln.split(":")[0] for ln in lines] == [
        "model_name", "parameters", "gflops", "seeds", "training_time_hours",
        "downstream_mlp_acc_image", "downstream_knn_accuracy_image",
        "downstream_mlp_acc_audio", "downstream_knn_accuracy_audio"]
    ckpts = [os.path.join(model_dir, f"simclr_seed{s}.ckpt") for s in (1, 2)]
    for s, ck in zip((1, 2), ckpts):
        assert os.path.isfile(ck)
        assert os.path.isfile(os.path.join(model_dir, "logs", f"version_seed{s}", "metrics.csv"))
        assert os.path.isfile(os.path.join(model_dir, "checkpoints", f"model_seed{s}.ckpt"))
    # per-seed accuracies = compute_train_results on the same trained weights
    for i, ck in enumerate(ckpts):
        m = MultiModalSimCLRLightning.load_from_checkpoint(ck)
        for mod in ("image", "audio"):
            knn, mlp, _ = T.compute_train_results(getattr(m.model, f"{mod}_encoder"), str(tmp_path / "chk"),
                                                  f"chk_{mod}", data.tr, data.va, data.te)
            assert knn == perf["per_seed"][mod]["knn"][i], (i, mod)
            assert mlp == perf["per_seed"][mod]["mlp"][i], (i, mod)
    knns = perf["per_seed"]["image"]["knn"]
    assert perf["downstream_knn_accuracy_image"] == f"{np.mean(knns):.4f} ± {np.std(knns):.4f}"
    summary = T.evaluate_multimodal_ssl(MultiModalSimCLRLightning, ckpts, data, "simclr")
    assert list(summary) == ["fusion", "downstream_knn_accuracy_fusion", "downstream_mlp_acc_fusion"]
    assert summary["fusion"] == "concat" and " ± " in summary["downstream_mlp_acc_fusion"]
    assert (tmp_path / "simclr_fusion_performance_summary.txt").read_text().splitlines()[0] == "fusion: concat"
