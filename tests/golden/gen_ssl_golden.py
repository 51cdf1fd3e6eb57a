"""Generate the SimCLR downstream fixtures ssl_downstream_{image,audio,fusion}[_f64].npz by
running the REFERENCE's own downstream functions on its own MultiModalSimCLRModel, on CPU.

Usage (only where /root/reference exists; the GPU box never runs this):
    python tests/golden/gen_ssl_golden.py [--out tests/golden] [--pseed N]

As gen_golden.py's downstream_case: placeholder modules for the absent third-party packages
are written to /tmp at run time (here also seaborn and optuna, which ssl_train.py's plotting
imports pull in); the reference's MultiModalSimCLRModel is filled from
oracle.params.make_state(ospec.simclr_spec(D, P), pseed); its train_knn_classifier,
train_downstream and compute_classification_metrics (training_structures/dino_train.py) run with
is_dino_based=False on
    image   model.image_encoder
    audio   model.audio_encoder
    fusion  LateFusionEncoder(audio_encoder, image_encoder, fusion="concat"), the reference's
            class imported from training_structures/ssl_train.py.
Harness-only changes, as there: DownstreamClassifier / FeatureExtractor are subclassed inside
dino_train's namespace to load the classifier from oracle/params.py and to cast the inputs to
the run dtype; dropout is set to 0.

Every target runs in float32 and in float64.  The float64 fixture also stores, per quantity,
the reference's own |f32 - f64| difference (``refdiff/...``): the GPU test's band is the larger
of test_gpu_downstream.py's constant and 4x that difference.  The seed is accepted only if the
two runs agree on every test row's kNN prediction, on the per-epoch validation accuracies and
on the test predictions (asserted here): the reference itself must not sit on a decision
boundary that f32 rounding moves."""
import argparse
import csv
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
from gen_golden import make_multimodal_batch, make_state, ospec  # noqa: E402

EXTRA_STUBS = {
    "seaborn/__init__.py": "",
    "optuna/__init__.py": "",
}

D, P, B = 32, 16, 16
NB_TRAIN, NB_VALID, NB_TEST, EPOCHS, LR = 3, 2, 2, 2, 1e-3
BSEED = 3021


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def run_target(target, dt, pseed):
    """One target in one dtype -> dict of raw results (numpy)."""
    import torch
    from torch.utils.data import DataLoader, TensorDataset
    import models.dino as rd
    import training_structures.dino_train as tdt
    import training_structures.ssl_train as rst
    sys.path.insert(0, os.path.join(G.REF, "other_ssl", "multimodal_simclr"))
    import multimodal_simclr as rs
    torch.use_deterministic_algorithms(False)      # set globally by the reference's imports
    dtt = getattr(torch, dt)
    torch.manual_seed(0)
    model = rs.MultiModalSimCLRModel(output_dim=D, projection_dim=P)
    spec = ospec.simclr_spec(D, P)
    G.load_into(model, spec, make_state(spec, pseed))
    G.zero_dropout(model)
    model = model.to(dtt)
    if target == "fusion":
        enc = rst.LateFusionEncoder(model.audio_encoder, model.image_encoder, fusion="concat")
    else:
        enc = getattr(model, f"{target}_encoder")
    cstate = make_state(ospec.classifier_spec(enc.output_dim), pseed + 1)

    class DC(rd.DownstreamClassifier):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.to(dtt)
            with torch.no_grad():
                for kk, v in cstate.items():
                    dict(self.named_parameters())[kk].copy_(torch.from_numpy(v).to(dtt))

        def forward(self, images, spectrograms=None):
            return super().forward(images.to(dtt), None if spectrograms is None else spectrograms.to(dtt))

    class FE(rd.FeatureExtractor):
        def forward(self, images, spectrograms=None):
            return super().forward(images.to(dtt), None if spectrograms is None else spectrograms.to(dtt))

    tdt.DownstreamClassifier, tdt.FeatureExtractor = DC, FE

    def loader(n, seed):
        bs = [make_multimodal_batch(B, 1, 0, seed + i) for i in range(n)]
        cat = lambda k: torch.from_numpy(np.concatenate([b[k] for b in bs]))  # noqa: E731
        return DataLoader(TensorDataset(cat("image"), cat("audio"), cat("label")), batch_size=B,
                          shuffle=False)

    tr, va, te = loader(NB_TRAIN, BSEED), loader(NB_VALID, BSEED + 1000), loader(NB_TEST, BSEED + 2000)
    r = {}
    knn, acc = tdt.train_knn_classifier(enc, tr, te, n_neighbors=5, device="cpu", is_dino_based=False)
    fe = FE(enc, is_dino_based=False)
    trf, _ = tdt.feature_extraction_loop("cpu", fe, tr)
    tef, _ = tdt.feature_extraction_loop("cpu", fe, te)
    r["knn_acc"] = np.float64(acc)
    r["knn_pred"] = knn.predict(tef).astype(np.int64)
    r["knn_nbr"] = knn.kneighbors(tef, return_distance=False).astype(np.int64)
    r["feat_train"], r["feat_test"] = np.asarray(trf, np.float64), np.asarray(tef, np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        clf = tdt.train_downstream(enc, tr, va, te, num_epochs=EPOCHS, device="cpu", learning_rate=LR,
                                   save_path=f"{tmp}/d/m.pt", train_log_path=f"{tmp}/d/train.csv",
                                   test_log_path=f"{tmp}/d/test.csv", is_dino_based=False)
        logs = sorted(os.listdir(f"{tmp}/d"))
        with open(f"{tmp}/d/" + [f for f in logs if f.startswith("train")][0]) as f:
            rows = list(csv.reader(f))[1:]
        r["history"] = np.array([[float(x[1]), float(x[2]), float(x[3])] for x in rows], np.float64)
        with open(f"{tmp}/d/" + [f for f in logs if f.startswith("test")][0]) as f:
            rows = list(csv.reader(f))[1:]
        r["test_preds"] = np.array([int(x[1]) for x in rows], np.int64)
        r["test_labels"] = np.array([int(x[0]) for x in rows], np.int64)
    met = tdt.compute_classification_metrics(clf, te, device="cpu")
    r["test_acc"] = np.float64(met["accuracy"])
    r["confusion_matrix"] = met["confusion_matrix"].astype(np.int64)
    for k, v in clf.named_parameters():
        if k.startswith("classifier"):
            r["cls/" + k] = v.detach().double().numpy()
    return r


def pack(r, target, pseed, store):
    G.STORE["dtype"] = store
    out = {"meta_dims": np.array([D, P, B, NB_TRAIN, NB_VALID, NB_TEST, EPOCHS, pseed, BSEED]),
           "meta_target": np.array(target), "meta_lr": np.float64(LR)}
    for k, v in r.items():
        if k.startswith(("feat_", "cls/")):
            G.summarize(k, v, out)
        else:
            out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--pseed", type=int, default=131)
    args = ap.parse_args()
    G.STUBS.update(EXTRA_STUBS)
    G.write_stubs()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for target in ("image", "audio", "fusion"):
        r32 = run_target(target, "float32", args.pseed)
        r64 = run_target(target, "float64", args.pseed)
        # the seed is usable only if the reference's own two precisions decide alike
        assert np.array_equal(r32["knn_pred"], r64["knn_pred"]), (target, "kNN predictions differ")
        assert np.array_equal(r32["history"][:, 2], r64["history"][:, 2]), (target, "val accuracy differs")
        assert np.array_equal(r32["test_preds"], r64["test_preds"]), (target, "test predictions differ")
        o32, o64 = pack(r32, target, args.pseed, np.float32), pack(r64, target, args.pseed, np.float64)
        o64["refdiff/feat_train"] = np.float64(rel(r32["feat_train"], r64["feat_train"]))
        o64["refdiff/feat_test"] = np.float64(rel(r32["feat_test"], r64["feat_test"]))
        o64["refdiff/history"] = np.float64(np.abs(r32["history"][:, :2] - r64["history"][:, :2]).max())
        o64["refdiff/cls"] = np.float64(max(rel(r32[k], r64[k]) for k in r64 if k.startswith("cls/")))
        name = f"ssl_downstream_{target}"
        np.savez_compressed(os.path.join(args.out, name + ".npz"), **o32)
        np.savez_compressed(os.path.join(args.out, name + "_f64.npz"), **o64)
        print(f"{name}: knn {float(r64['knn_acc']):.2f}% history {r64['history'].tolist()} "
              f"test {float(r64['test_acc']):.2f}% refdiff feat {float(o64['refdiff/feat_train']):.2e} "
              f"hist {float(o64['refdiff/history']):.2e} cls {float(o64['refdiff/cls']):.2e}")


if __name__ == "__main__":
    main()
