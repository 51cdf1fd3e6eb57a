"""``training_structures/dino_train.py`` of the reference on the MI355X engine.

  pretrain_dino                 dino_train.py:104-186   the training_structures DINO loop
                                (BASELINE config 1's path): AdamW(lr) with torch's default
                                weight_decay 0.01, per batch zero_grad -> forward -> dino_loss
                                -> backward -> step -> update_teacher (EMA AFTER the step),
                                per-epoch CSV log and best-loss checkpoint
  dino_loss / unimodal_dino_loss the loss callables pretrain_dino takes (the Lightning modules'
                                dino_loss, dino.py:822-854 / 1596-1635, as free functions)
  train_downstream, train_knn_classifier, feature_extraction_loop,
  compute_classification_metrics, compute_accuracies    -> avdino.downstream (re-exported)

and ``training_structures/ssl_train.py`` (the SimCLR experiment, BASELINE config 4):

  compute_train_results         ssl_train.py:19-42     kNN (k=5) + 10-epoch MLP on one encoder
  train_and_evaluate_ssl        ssl_train.py:75-243    per seed: fit, checkpoint, evaluate the
                                towers; ``{model_name}_performance_summary.txt``
  LateFusionEncoder             ssl_train.py:245-292   concat / sum / mean of the two towers
  evaluate_multimodal_ssl       ssl_train.py:294-359   late-fusion accuracies over checkpoints

Out of scope there: the plots (visualize_results: PCA, t-SNE, confusion figures, loss curves).
The SimCLR augmentation data module is avdino.data.AVMNISTSimCLRDataModule.

Deviation, documented: the reference's pretrain_dino unpacks ``student_out, teacher_out =
model(batch)``, while its current models return three values (dino.py:727, 1398) and would
raise there; this loop takes the first two.  ``align=True`` needs a model exposing
``student.loss_align`` (the reference's archived alignment encoders), none of which is on the
hot path.
"""
import csv
import json
import os
from datetime import datetime

import numpy as np
import torch

from .downstream import (compute_accuracies, compute_classification_metrics,  # noqa: F401
                         feature_extraction_loop, train_downstream, train_knn_classifier)
from .models import FlatAdam, _DinoLossFn


def dino_loss(student_outputs, teacher_outputs, alignment_loss=None, tau_s=0.1, tau_t=0.04):
    """MultiModalDINOLightning.dino_loss (dino.py:822-854) as a free function: fused HIP
    kernel, differentiable w.r.t. student_outputs."""
    loss = _DinoLossFn.apply(student_outputs, teacher_outputs, tau_s, tau_t, False)
    return loss if alignment_loss is None else loss + alignment_loss


def unimodal_dino_loss(student_outputs, teacher_outputs, tau_s=0.1, tau_t=0.04):
    """UniModalDINOLightning.dino_loss (dino.py:1596-1635): the teacher additionally centred
    by its per-view batch mean."""
    return _DinoLossFn.apply(student_outputs, teacher_outputs, tau_s, tau_t, True)


def _stamp(path, stamp):
    return path.replace(".pt", f"_{stamp}.pt") if path.endswith(".pt") else \
        path.replace(".csv", f"_{stamp}.csv")


def pretrain_dino(model, trainloader, dino_loss, align=False, num_epochs=100, learning_rate=0.0001,
                  save_path="pretrained_dino.pt", log_path="pretrain_log.csv", write_logs=True):
    """dino_train.py:104-186 -> the trained model (``model.epoch_losses`` holds the per-epoch
    means, ``model.step_losses`` the per-step losses as one device tensor per epoch)."""
    if align:
        raise NotImplementedError("align=True needs an alignment encoder (not on the hot path)")
    opt = FlatAdam(model.trainable_arenas(), lr=learning_rate, weight_decay=0.01, decoupled=True)
    stamp = datetime.now().strftime("%Y-%m-%d %H-%M-%S")
    if write_logs:
        for path in (save_path, log_path):
            d = os.path.dirname(path)
            if d:
                os.makedirs(d, exist_ok=True)
        save_path, log_path = _stamp(save_path, stamp), _stamp(log_path, stamp)
        info = {"start_time": stamp, "learning_rate": learning_rate,
                "batch_size": getattr(trainloader, "batch_size", None), "epochs": num_epochs,
                "model_name": "MultiModalDINO"}
        with open(log_path, "w", newline="") as f:
            csv.writer(f).writerow(["epoch", "train_loss", f"# {json.dumps(info)}"])
    best = float("inf")
    model.epoch_losses, model.step_losses = [], []
    for epoch in range(num_epochs):
        model.train()
        losses = []
        for batch in trainloader:
            opt.zero_grad()
            student_out, teacher_out = model(tuple(batch[:4]))[:2]
            loss = dino_loss(student_out, teacher_out, tau_s=0.1, tau_t=0.04)
            loss.backward()
            opt.step()
            model.update_teacher()       # EMA of the post-step student
            losses.append(loss.detach().reshape(1))
        step = torch.cat(losses)
        avg = step.mean().item()
        model.step_losses.append(step)
        model.epoch_losses.append(avg)
        if write_logs:
            with open(log_path, "a", newline="") as f:
                csv.writer(f).writerow([epoch + 1, avg])
        if avg < best:
            best = avg
            if write_logs:
                torch.save({"epoch": epoch, "model_state_dict": {k: v.detach().cpu() for k, v in
                                                                 model.state_dict().items()},
                            "optimizer_state_dict": opt.state_dict(), "loss": best}, save_path)
    return model


# ============================================================================ ssl_train.py
def compute_train_results(pretrained_model, model_path, model_name, traindata, validdata, testdata):
    """ssl_train.py:19-42 -> (knn accuracy %, mlp accuracy %, classifier): kNN (k = 5) and the
    10-epoch MLP probe on a frozen copy of ``pretrained_model`` -- a SimCLR tower
    (``model.image_encoder`` / ``model.audio_encoder``) or a LateFusionEncoder."""
    store = (pretrained_model.image_encoder if hasattr(pretrained_model, "fusion")
             else pretrained_model).store
    device = store.device
    _, knn_accuracy = train_knn_classifier(pretrained_model, traindata, testdata, n_neighbors=5,
                                           device=device, is_dino_based=False)
    classifier = train_downstream(
        pretrained_model, traindata, validdata, testdata, num_epochs=10, device=device,
        save_path=f"{model_path}/downstream/{model_name}.pt",
        train_log_path=f"{model_path}/downstream/{model_name}_train_log.csv",
        test_log_path=f"{model_path}/downstream/{model_name}_test_log.csv",
        is_dino_based=False)
    mlp_accuracy = compute_classification_metrics(classifier, testdata, device)["accuracy"]
    return knn_accuracy, mlp_accuracy, classifier


class LateFusionEncoder:
    """Late fusion of two pretrained towers (ssl_train.py:245-292) for the downstream
    functions: features = cat([image, audio], 1) ("concat"), their sum or their mean.
    ``output_dim`` is the sum of the towers' dims for concat, their common dim otherwise.  The
    reference's ``proj_dim`` puts an untrained random Linear behind the fusion; that is not
    carried here."""

    def __init__(self, audio_encoder, image_encoder, fusion="concat", proj_dim=None):
        if fusion not in ("concat", "sum", "mean"):
            raise ValueError(f"Unknown fusion strategy: {fusion}")
        if proj_dim is not None:
            raise NotImplementedError("proj_dim: the reference's projection is an untrained random "
                                      "Linear; only proj_dim=None is supported")
        da, di = audio_encoder.output_dim, image_encoder.output_dim
        if fusion != "concat" and da != di:
            raise ValueError(f"fusion={fusion!r} needs towers of one width, got {da} and {di}")
        self.audio_encoder, self.image_encoder = audio_encoder, image_encoder
        self.fusion, self.proj = fusion, None
        self.output_dim = da + di if fusion == "concat" else da

    def parameters(self):
        yield from self.audio_encoder.parameters()


def ssl_model_stats(model):
    """(GFLOPs, parameter count) of a MultiModalSimCLRModel for the performance summary.
    ``parameters`` is the true count of the state dict's parameter tensors; ``gflops`` is
    analytic, as run_dino.model_stats: the Conv2d / Linear multiply-adds of one (image,
    spectrogram) pair through both towers and both projection heads.  The reference measures it
    with a profiler package on a randomly drawn modality pair, so this figure is NOT pinned to
    the reference's."""
    import math

    from .run_dino import _stack_macs
    from .spec import UNI_ENCODERS
    spec = model.store.spec
    params = sum(int(math.prod(shp)) for _k, (shp, kind) in spec.items()
                 if kind in ("w", "b", "bn_w", "bn_b"))

    def lin(key):
        shp = spec[key + ".weight"][0]
        return shp[0] * shp[1]

    macs = 0
    for h in (model.image_encoder, model.audio_encoder):
        _mod, stack, lins, _sd = UNI_ENCODERS[h.kind]
        macs += _stack_macs(stack(h.prefix)) + sum(lin(f"{h.prefix}.{k}") for k in lins)
        macs += lin(f"{h.prefix[:-len('_encoder')]}_projection_head.mlp.0")
        macs += lin(f"{h.prefix[:-len('_encoder')]}_projection_head.mlp.4")
    return macs / 1e9, params


def _mean_std(values):
    return f"{np.mean(values):.4f} \u00b1 {np.std(values):.4f}"


def write_ssl_summary(path, model_name, params, gflops, seeds, training_times, accuracies):
    """``{model_name}_performance_summary.txt`` (ssl_train.py:205-223): key: value lines.
    accuracies: {"image": (knn list, mlp list), "audio": (...)} for the evaluated modalities, in
    the reference's order (image first).  Returns the dict written."""
    perf = {"model_name": model_name, "parameters": f"{params / 1e6:.2f}M", "gflops": f"{gflops:.2f}",
            "seeds": list(seeds), "training_time_hours": f"{np.mean(training_times) / 3600:.2f}"}
    for mod in ("image", "audio"):
        if mod in accuracies:
            knn, mlp = accuracies[mod]
            perf[f"downstream_mlp_acc_{mod}"] = _mean_std(mlp)
            perf[f"downstream_knn_accuracy_{mod}"] = _mean_std(knn)
    with open(path, "w") as f:
        for key, value in perf.items():
            f.write(f"{key}: {value}\n")
    return perf


def train_and_evaluate_ssl(module, train_data_module, test_data_module, model_dir, model_name,
                           input_data=None, modalities=["audio", "image"], seeds=[1, 2, 3],
                           num_epochs=100):
    """ssl_train.py:75-243: for every seed restore the initial weights, seed the run, fit
    ``module`` (this project's Trainer with CSVLogger(model_dir, "logs", f"version_seed{seed}")
    and ModelCheckpoint(monitor="train_loss")), save ``{model_dir}/{model_name}_seed{seed}.ckpt``
    and evaluate the requested towers (compute_train_results on test_data_module's loaders); then
    write ``{model_name}_performance_summary.txt`` (mean and population std over the seeds).

    train_data_module: a data module (``train_dataloader()``) or a loader yielding
    (img1, spec1, img2, spec2); test_data_module: ``setup()``, ``train_dataloader()``,
    ``val_dataloader()``, ``test_dataloader()`` yielding (image, audio, label).  ``input_data``
    is accepted for signature parity and unused: parameters / gflops come from ssl_model_stats
    (gflops analytic, not pinned to the reference's profiler figure).  Returns the summary dict
    (``per_seed`` added: the per-seed accuracies).  Not mirrored: the plots (module
    docstring)."""
    import copy
    import time

    from .run_dino import _set_seed
    from .trainer import CSVLogger, ModelCheckpoint, Trainer
    os.makedirs(model_dir, exist_ok=True)
    test_data_module.setup()
    initial = copy.deepcopy({k: v.detach().clone() for k, v in module.state_dict().items()})
    gflops, params = ssl_model_stats(module.model)
    acc = {m: ([], []) for m in ("image", "audio") if m in modalities}
    times = []
    for seed in seeds:
        print(f"Training with seed {seed}...")
        _set_seed(seed)
        module.load_state_dict(copy.deepcopy(initial))
        logger = CSVLogger(f"{model_dir}", name="logs", version=f"version_seed{seed}")
        checkpoint = ModelCheckpoint(monitor="train_loss", dirpath=f"{model_dir}/checkpoints/",
                                     filename=f"model_seed{seed}", save_top_k=1, mode="min")
        t0 = time.time()
        trainer = Trainer(max_epochs=num_epochs, devices=1,
                          precision="16-mixed" if module.use_mixed_precision else 32,
                          callbacks=[checkpoint], logger=logger)
        if hasattr(train_data_module, "train_dataloader"):
            trainer.fit(module, datamodule=train_data_module)
        else:
            trainer.fit(module, train_data_module)
        times.append(time.time() - t0)
        trainer.save_checkpoint(f"{model_dir}/{model_name}_seed{seed}.ckpt")
        for mod in ("audio", "image"):
            if mod not in acc:
                continue
            knn, mlp, _clf = compute_train_results(
                getattr(module.model, f"{mod}_encoder"), model_dir, f"{model_name}_{mod}",
                test_data_module.train_dataloader(), test_data_module.val_dataloader(),
                test_data_module.test_dataloader())
            acc[mod][0].append(knn)
            acc[mod][1].append(mlp)
            print(f"{mod.capitalize()} KNN Accuracy: {knn}, MLP Accuracy: {mlp}")
    perf = write_ssl_summary(f"{model_name}_performance_summary.txt", model_name, params, gflops,
                             seeds, times, acc)
    perf["per_seed"] = {m: {"knn": list(v[0]), "mlp": list(v[1])} for m, v in acc.items()}
    return perf


def evaluate_multimodal_ssl(lightning_cls, ckpt_paths, test_data_module, model_name,
                            fusion="concat", proj_dim=None):
    """ssl_train.py:294-359: late fusion of the two towers of every checkpoint ->
    {"fusion", "downstream_knn_accuracy_fusion", "downstream_mlp_acc_fusion"} (mean and
    population std over the checkpoints), also written to
    ``{model_name}_fusion_performance_summary.txt``.  The plots are not mirrored."""
    test_data_module.setup()
    knns, mlps = [], []
    for ckpt_path in ckpt_paths:
        print(f"Loading checkpoint {ckpt_path}...")
        module = lightning_cls.load_from_checkpoint(ckpt_path)
        enc = LateFusionEncoder(module.model.audio_encoder, module.model.image_encoder,
                                fusion=fusion, proj_dim=proj_dim)
        knn, mlp, _clf = compute_train_results(
            pretrained_model=enc, model_path=".", model_name=f"{model_name}_fusion",
            traindata=test_data_module.train_dataloader(), validdata=test_data_module.val_dataloader(),
            testdata=test_data_module.test_dataloader())
        knns.append(knn)
        mlps.append(mlp)
        print(f"Fusion KNN Accuracy: {knn}, MLP Accuracy: {mlp}")
    summary = {"fusion": fusion, "downstream_knn_accuracy_fusion": _mean_std(knns),
               "downstream_mlp_acc_fusion": _mean_std(mlps)}
    with open(f"{model_name}_fusion_performance_summary.txt", "w") as f:
        for k, v in summary.items():
            f.write(f"{k}: {v}\n")
    return summary
