"""Golden vectors of the audio CNN+LSTM encoder, made by running the REFERENCE's own
UniModalDINO(encoder_class=SpectrogramEncoderLSTM) (models/dino.py:117-156, 525-530, 1257-1398)
on the CPU in fp32 and float64, replaying UniModalDINOLightning.training_step (1637-1668) and
Adam, exactly as gen_golden.py's unimodal_case does for the other encoders.

Usage (only where the reference checkout exists; the GPU tests never run this):
    python tests/golden/gen_lstm_golden.py [--out tests/golden]

Writes ``uni_speclstm_g2l2.npz`` / ``_f64.npz`` (3 steps: loss, outputs, embeddings, every
gradient, EMA'd teacher, running statistics, post-Adam parameters of step 0, and the loss
curve), ``speclstm_eval_features[_f64].npz`` (eval-mode student features of two loader batches,
the second ragged) and ``lstm_state_keys.json`` (the reference's state_dict keys and shapes, in
order).  Parameters come from tests/lstm_ref.py lstm_state by key, so the fixtures hold outputs
only.  Dimensions and seeds: tests/lstm_ref.py.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "multimodal-ssl-avmnist_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden  # noqa: E402
from gen_golden import STORE, load_into, summarize, write_stubs, zero_dropout  # noqa: E402
from oracle.params import make_multimodal_batch  # noqa: E402
from tests import lstm_ref as LR  # noqa: E402

# tensors above this many elements are stored as (sum, norm, sampled entries)
gen_golden.FULL_MAX = 4096
# every feature_proj / lstm gradient must be well away from zero in float64: the tests take the
# relative check on all of them
MIN_GRAD_NORM = 1e-4


def _model(pseed, dt, stats=False):
    import torch
    import models.dino as rd
    D, P = LR.DIMS["D"], LR.DIMS["P"]
    torch.manual_seed(0)
    model = rd.UniModalDINO(encoder_class=rd.SpectrogramEncoderLSTM, output_dim=D, projection_dim=P,
                            momentum=LR.HP["momentum"], center_momentum=LR.HP["center_momentum"],
                            dropout=0.0)
    spec = LR.lstm_spec(D, P)
    load_into(model, spec, LR.lstm_state(spec, pseed, stats=stats))
    zero_dropout(model)
    return rd, model.to(dt)


def step_case(name, out_dir, dt):
    import torch
    f64 = dt == "float64"
    dt = getattr(torch, dt)
    D, P, B, G, L = (LR.DIMS[k] for k in "DPBGL")
    rd, model = _model(LR.PSEED, dt)
    model.train()
    selfns = types.SimpleNamespace(student_temperature=LR.HP["tau_s"], teacher_temperature=LR.HP["tau_t"])
    opt = torch.optim.Adam(model.parameters(), lr=LR.HP["lr"], weight_decay=LR.HP["wd"])
    out = {"meta_dims": np.array([D, P, B, G, L, LR.PSEED, LR.BSEED]), "meta_modality": np.array(LR.KIND),
           "meta_cos_alpha": np.float64(0.0)}
    curve = []
    for step in range(LR.STEPS):
        b = make_multimodal_batch(B, G, L, LR.BSEED + step, with_originals=False)
        t = {k: torch.from_numpy(v).to(dt) for k, v in b.items()}
        s_out, t_out, emb = model((t["g_img"], t["g_aud"], t["l_img"], t["l_aud"]))
        loss = rd.UniModalDINOLightning.dino_loss(selfns, s_out, t_out)
        model.update_teacher()
        opt.zero_grad()
        loss.backward()
        if step == 0:
            out["loss"] = np.float64(loss.item())
            summarize("s_out", s_out.detach().numpy(), out)
            summarize("t_out", t_out.detach().numpy(), out)
            summarize("emb", emb.detach().numpy(), out)
            for k, p in model.named_parameters():
                if p.grad is not None:
                    summarize("grad/" + k, p.grad.numpy(), out)
                    if f64 and ("feature_proj" in k or ".lstm." in k):
                        n = float(p.grad.norm())
                        assert n >= MIN_GRAD_NORM, f"{k}: |grad| = {n:.3g}: pick other seeds"
            out["live_keys"] = np.array([k for k, p in model.named_parameters() if p.grad is not None])
        opt.step()
        if step == 0:
            for k, v in model.state_dict().items():
                if k.endswith("running_mean") or k.endswith("running_var"):
                    summarize("rs/" + k, v.numpy(), out)
                elif k == "center":
                    out["center_after"] = v.numpy().astype(STORE["dtype"])
                elif k.startswith("teacher") and not k.endswith("num_batches_tracked"):
                    summarize("ema/" + k, v.numpy(), out)
                elif not k.endswith("num_batches_tracked"):
                    summarize("post/" + k, v.numpy(), out)
        curve.append(loss.item())
    out["curve"] = np.array(curve, np.float64)
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **out)
    print(f"{name}: loss={out['loss']:.8f} curve={np.array(curve)}")


def eval_case(name, out_dir, dt):
    import torch
    dt = getattr(torch, dt)
    _rd, model = _model(LR.PSEED, dt, stats=True)
    model.eval()
    out = {"meta_dims": np.array([LR.DIMS["D"], LR.DIMS["P"], LR.PSEED, LR.EVAL_SEED]),
           "meta_batches": np.array(LR.EVAL_BATCHES)}
    with torch.no_grad():
        for i, n in enumerate(LR.EVAL_BATCHES):
            b = make_multimodal_batch(n, 1, 1, LR.EVAL_SEED + i)
            f = model.student(images=None, spectrograms=torch.from_numpy(b["audio"]).to(dt))
            out[f"feat{i}"] = f.numpy().astype(STORE["dtype"])
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **out)
    print(f"{name}: |feat0|={np.linalg.norm(out['feat0']):.6f}")


def key_list(out_dir):
    import torch
    _rd, model = _model(1, torch.float32)
    keys = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(out_dir, "lstm_state_keys.json"), "w") as f:
        json.dump({f"{LR.KIND}/D{LR.DIMS['D']}_P{LR.DIMS['P']}": keys}, f, indent=0)
    print("lstm_state_keys.json:", len(keys), "keys")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    write_stubs()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    key_list(args.out)
    for dt, sfx, store in (("float32", "", np.float32), ("float64", "_f64", np.float64)):
        STORE["dtype"] = store
        step_case(LR.NAME + sfx, args.out, dt)
        eval_case(LR.EVAL_NAME + sfx, args.out, dt)


if __name__ == "__main__":
    main()
