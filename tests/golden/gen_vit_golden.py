"""Golden vectors of the audio ViT encoder, made by running the REFERENCE's own
UniModalDINO(encoder_class=SpectrogramEncoderViT) (models/dino.py:532-546, 1257-1398;
models/dino_vit.py:27-63, 122-177) on the CPU in fp32 and float64, replaying
UniModalDINOLightning.training_step (1637-1668) and Adam, exactly as gen_lstm_golden.py does for
the CNN+LSTM encoder.

Usage (only where the reference checkout exists; the GPU tests never run this):
    python tests/golden/gen_vit_golden.py [--out tests/golden]

Writes ``uni_specvit_g2l2.npz`` / ``_f64.npz`` (3 steps: loss, outputs, embeddings, every
gradient -- the attention in-projection's also per q / k / v slice, ``grad/<key>#q`` ... --
EMA'd teacher, running statistics, post-Adam parameters of step 0, and the loss curve),
``specvit_eval_features[_f64].npz`` (eval-mode student features of two loader batches, the second
ragged) and ``vit_state_keys.json`` (the reference's state_dict keys and shapes, in order).
Parameters come from tests/vit_ref.py vit_state by key, so the fixtures hold outputs only.
Dimensions and seeds: tests/vit_ref.py.

Dropout off = every nn.Dropout at p = 0 AND nn.MultiheadAttention.dropout = 0.0 (a float
attribute handed to the attention function, not an nn.Dropout module).

Two conditions are asserted in float64 (pick other seeds or another ATTN_SCALE if either fails):
the mean over query rows of the largest attention probability lies in [0.05, 0.9] in every layer,
and every ViT parameter gradient has norm >= 1e-4, in_proj_weight / in_proj_bias per q / k / v
slice -- except the mathematically zero ones, which must be below 1e-12: the k slice of
in_proj_bias (a constant added to every key's score leaves the softmax unchanged), and the final
LayerNorm's bias and the Linear(512, D) bias behind it (a constant added to every row of the
projection head's train-mode BatchNorm1d input; tests/vit_ref.py ZERO_BN_BIAS).
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
from tests import vit_ref as VR  # noqa: E402

# tensors above this many elements are stored as (sum, norm, 128 sampled entries): the tower has
# some 60 parameter tensors of 512 elements and more, each stored three times (gradient, EMA'd
# teacher, post-Adam), and the float64 file must stay well under the size limit of a committed file
gen_golden.FULL_MAX = 256
gen_golden.SAMPLE = 128
MIN_GRAD_NORM = 1e-4
MAXPROB = (0.05, 0.9)


def _model(pseed, dt, stats=False):
    import torch
    import torch.nn as nn
    import models.dino as rd
    D, P = VR.DIMS["D"], VR.DIMS["P"]
    torch.manual_seed(0)
    model = rd.UniModalDINO(encoder_class=rd.SpectrogramEncoderViT, output_dim=D, projection_dim=P,
                            momentum=VR.HP["momentum"], center_momentum=VR.HP["center_momentum"],
                            dropout=0.0)
    spec = VR.vit_spec(D, P)
    load_into(model, spec, VR.vit_state(spec, pseed, stats=stats))
    zero_dropout(model)
    n = 0
    for m in model.modules():
        if isinstance(m, nn.MultiheadAttention):
            m.dropout = 0.0
            n += 1
    assert n == 2 * VR.DEPTH, n
    return rd, model.to(dt)


def _slices(k, g):
    """(suffix, array) of a gradient: the whole tensor, and q / k / v thirds of an in-projection."""
    out = [("", g)]
    if "in_proj_" in k:
        E = g.shape[0] // 3
        out += [("#" + n, g[i * E:(i + 1) * E]) for i, n in enumerate("qkv")]
    return out


def check_conditions(grads):
    """The two float64 conditions of the module docstring (grads: student key -> ndarray)."""
    D, P, B, G, L = (VR.DIMS[k] for k in "DPBGL")
    spec = VR.vit_spec(D, P)
    probs = []
    r = VR.unimodal_step(VR.vit_state(spec, VR.PSEED), make_multimodal_batch(B, G, L, VR.BSEED, with_originals=False),
                         VR.HP, spec, probs=probs)
    per_layer = np.array(probs).reshape(-1, VR.DEPTH).mean(axis=0)    # calls x layers
    print("mean largest attention probability per layer:", per_layer)
    assert all(MAXPROB[0] <= v <= MAXPROB[1] for v in per_layer), per_layer
    for k, g in grads.items():
        for sfx, a in VR.grad_slices(k, g):
            n = float(np.linalg.norm(a))
            if VR.is_zero_grad(k, sfx):
                print(f"{k}{sfx}: |grad| = {n:.3g} (mathematically zero)")
                assert n < 1e-12, (k, n)
            elif ".encoder." in k:
                assert n >= MIN_GRAD_NORM, f"{k}{sfx}: |grad| = {n:.3g}: pick other seeds or scales"


def step_case(name, out_dir, dt):
    import torch
    f64 = dt == "float64"
    dt = getattr(torch, dt)
    D, P, B, G, L = (VR.DIMS[k] for k in "DPBGL")
    rd, model = _model(VR.PSEED, dt)
    model.train()
    selfns = types.SimpleNamespace(student_temperature=VR.HP["tau_s"], teacher_temperature=VR.HP["tau_t"])
    opt = torch.optim.Adam(model.parameters(), lr=VR.HP["lr"], weight_decay=VR.HP["wd"])
    out = {"meta_dims": np.array([D, P, B, G, L, VR.PSEED, VR.BSEED]), "meta_modality": np.array(VR.KIND),
           "meta_cos_alpha": np.float64(0.0), "meta_attn_scale": np.float64(VR.ATTN_SCALE)}
    curve = []
    for step in range(VR.STEPS):
        b = make_multimodal_batch(B, G, L, VR.BSEED + step, with_originals=False)
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
            grads = {k: p.grad.numpy() for k, p in model.named_parameters() if p.grad is not None}
            for k, g in grads.items():
                for sfx, a in _slices(k, g):
                    summarize("grad/" + k + sfx, a, out)
            if f64:
                check_conditions(grads)
            out["live_keys"] = np.array(list(grads))
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
    _rd, model = _model(VR.PSEED, dt, stats=True)
    model.eval()
    out = {"meta_dims": np.array([VR.DIMS["D"], VR.DIMS["P"], VR.PSEED, VR.EVAL_SEED]),
           "meta_batches": np.array(VR.EVAL_BATCHES)}
    with torch.no_grad():
        for i, n in enumerate(VR.EVAL_BATCHES):
            b = make_multimodal_batch(n, 1, 1, VR.EVAL_SEED + i)
            f = model.student(images=None, spectrograms=torch.from_numpy(b["audio"]).to(dt))
            out[f"feat{i}"] = f.numpy().astype(STORE["dtype"])
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **out)
    print(f"{name}: |feat0|={np.linalg.norm(out['feat0']):.6f}")


def key_list(out_dir):
    import torch
    _rd, model = _model(1, torch.float32)
    keys = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(out_dir, "vit_state_keys.json"), "w") as f:
        json.dump({f"{VR.KIND}/D{VR.DIMS['D']}_P{VR.DIMS['P']}": keys}, f, indent=0)
    print("vit_state_keys.json:", len(keys), "keys")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    write_stubs()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    key_list(args.out)
    for dt, sfx, store in (("float64", "_f64", np.float64), ("float32", "", np.float32)):
        STORE["dtype"] = store
        step_case(VR.NAME + sfx, args.out, dt)
        eval_case(VR.EVAL_NAME + sfx, args.out, dt)


if __name__ == "__main__":
    main()
