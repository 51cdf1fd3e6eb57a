"""Float64 restatement, in plain torch on the CPU, of SpectrogramEncoderLSTM and of one
UniModalDINO + UniModalDINOLightning training step over it (models/dino.py:117-156, 525-530,
1240-1398, 1596-1668): conv2d / batch_norm / nn.LSTM / autograd in float64.

tests/test_lstm_cpu.py pins it to the reference's float64 fixtures (tests/golden/
uni_speclstm_g2l2_f64.npz, made by tests/golden/gen_lstm_golden.py) to 1e-8, so the GPU tests
can use it as the yardstick where the reference itself does not exist.

Parameters are a pure function of (seed, state-dict key) -- oracle.params.make_tensor, as
tests/fusion_util.py -- so the fixtures hold outputs only.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle.params import make_tensor

KIND = "spectrogram_lstm"
# the fixture case: D = 32 (H = 16), P = 16, B = 3, 2 global + 2 local views, 3 steps
NAME = "uni_speclstm_g2l2"
DIMS = dict(D=32, P=16, B=3, G=2, L=2)
PSEED, BSEED, STEPS = 733, 7330, 3
# eval-mode student features of two loader batches, the second ragged
EVAL_NAME, EVAL_BATCHES, EVAL_SEED = "speclstm_eval_features", (4, 3), 7400
HP = dict(lr=1e-4, wd=1e-6, momentum=0.996, center_momentum=0.9, tau_s=0.1, tau_t=0.04)

# avdino.spec kinds -> oracle.params kinds (the LSTM tensors: matrices as dense weights, i.e.
# U(+-1/sqrt(columns)), vectors as dense biases, U(+-0.1) -- so b_ih != b_hh and neither is 0)
_KIND = {"w": "dense_w", "b": "dense_b", "bn_w": "bn_w", "bn_b": "bn_b", "rm": "rm", "rv": "rv",
         "nbt": "nbt", "center": "center"}


def lstm_spec(D, P):
    from avdino.spec import unimodal_dino_sd
    return unimodal_dino_sd(KIND, D, P)


def lstm_state(spec, seed, stats=False):
    """key -> ndarray.  stats: running statistics away from (0, 1), for the eval-mode fixture."""
    out = OrderedDict()
    for k, (shp, kind) in spec.items():
        if kind == "lstm":
            kind = "w" if len(shp) == 2 else "b"
        okind = _KIND[kind]
        if stats and kind in ("rm", "rv"):
            okind = "bn_b" if kind == "rm" else "bn_w"
        out[k] = make_tensor(seed, k, shp, okind)
    return out


def audio_views(batch):
    """[V, B, 1, 112, 112] float64: the global views, then the local ones."""
    g, l = batch["g_aud"], batch["l_aud"]
    v = np.concatenate([g, l], axis=1) if l.shape[1] else g
    return torch.from_numpy(np.ascontiguousarray(v.transpose(1, 0, 2, 3, 4))).double()


LSTM_NAMES = [n + s for s in ("", "_reverse")
              for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


def encoder(p, prefix, x, train):
    """One call of the encoder on x [B, 1, 112, 112]; p: key -> float64 tensor (running
    statistics are updated in place when train)."""
    e = prefix + ".encoder."
    h = x
    for i in (0, 4, 8):
        h = F.conv2d(h, p[f"{e}cnn.{i}.weight"], p[f"{e}cnn.{i}.bias"], padding=1)
        bn = f"{e}cnn.{i + 1}."
        h = F.batch_norm(h, p[bn + "running_mean"], p[bn + "running_var"], p[bn + "weight"],
                         p[bn + "bias"], training=train, momentum=0.1, eps=1e-5)
        h = F.max_pool2d(F.relu(h), 2)
    B, C = h.shape[:2]
    tok = h.view(B, C, -1).transpose(1, 2)
    xp = F.relu(F.linear(tok, p[e + "feature_proj.0.weight"], p[e + "feature_proj.0.bias"]))
    H = p[e + "lstm.weight_hh_l0"].shape[1]
    lstm = torch.nn.LSTM(xp.shape[-1], H, batch_first=True, bidirectional=True).double()
    return _lstm(lstm, p, e, xp).mean(dim=1)


def _lstm(mod, p, e, xp):
    """nn.LSTM forward with the caller's tensors as its weights (torch.func.functional_call)."""
    params = {n: p[e + "lstm." + n] for n in LSTM_NAMES}
    out, _ = torch.func.functional_call(mod, params, (xp,))
    return out


def head(p, prefix, x, train):
    m = prefix + ".mlp."
    h = F.linear(x, p[m + "0.weight"], p[m + "0.bias"])
    h = F.batch_norm(h, p[m + "1.running_mean"], p[m + "1.running_var"], p[m + "1.weight"],
                     p[m + "1.bias"], training=train, momentum=0.1, eps=1e-5)
    return F.linear(F.gelu(h), p[m + "4.weight"], p[m + "4.bias"])


def dino_loss(s_out, t_out, tau_s, tau_t):
    s = F.normalize(s_out, p=2, dim=-1)
    t = F.normalize(t_out, p=2, dim=-1)
    t = t - t.mean(dim=1, keepdim=True)
    tp = F.softmax(t / tau_t, dim=-1)
    sp = F.log_softmax(s / tau_s, dim=-1)
    total = 0
    for i in range(s.shape[0]):
        for j in range(t.shape[0]):
            total = total + -(tp[j] * sp[i]).sum(dim=-1).mean()
    return total / (s.shape[0] * t.shape[0])


def _is_param(spec, k):
    return spec[k][1] in ("w", "b", "bn_w", "bn_b", "lstm")


def unimodal_step(state, batch, hp, spec):
    """One training step up to (not including) Adam.  state: key -> ndarray.  Returns loss,
    s_out [V,B,P], t_out [G,B,P] (centred by the pre-update centre), emb [V,B,D], grads of the
    live student parameters, and ``state``: the state after the forward's buffer updates
    (running statistics, centre) and the teacher EMA -- student parameters unchanged."""
    p = OrderedDict()
    for k, v in state.items():
        t = torch.from_numpy(np.array(v))
        p[k] = t.double() if t.is_floating_point() else t.clone()
    live = [k for k in p if _is_param(spec, k) and k.startswith("student")]
    for k in live:
        p[k].requires_grad_(True)
    x = audio_views(batch)
    V, G = x.shape[0], batch["g_aud"].shape[1]
    B = x.shape[1]
    emb = torch.cat([encoder(p, "student", x[v], True) for v in range(V)])
    with torch.no_grad():
        temb = torch.cat([encoder(p, "teacher", x[v], True) for v in range(G)])
    s_proj = head(p, "student_projection", emb, True)
    with torch.no_grad():
        t_proj = head(p, "teacher_projection", temb, True)
        t_c = t_proj - p["center"]
        center_after = p["center"] * hp["center_momentum"] + \
            t_proj.mean(dim=0, keepdim=True) * (1 - hp["center_momentum"])
    s_out, t_out = s_proj.view(V, B, -1), t_c.view(G, B, -1)
    loss = dino_loss(s_out, t_out, hp["tau_s"], hp["tau_t"])
    loss.backward()
    grads = {k: p[k].grad.numpy().copy() for k in live if p[k].grad is not None}
    new = OrderedDict((k, v.detach().numpy().copy()) for k, v in p.items())
    new["center"] = center_after.numpy()
    m = hp["momentum"]
    for k in live:
        tk = "teacher" + k[len("student"):]
        new[tk] = m * new[tk] + (1 - m) * new[k]
    for k in new:
        if k.endswith("num_batches_tracked"):     # the encoder runs once per view, a head once
            new[k] = new[k] + (1 if "_projection." in k else V if k.startswith("student.") else G)
    return dict(loss=float(loss.item()), s_out=s_out.detach().numpy(), t_out=t_out.numpy(),
                emb=emb.detach().view(V, B, -1).numpy(), grads=grads, state=new,
                center_after=center_after.numpy())


def adam_update(state, grads, opt, t, hp):
    """torch.optim.Adam(lr, weight_decay = L2) on the keys of ``grads``; opt: key -> (m, v)."""
    out = OrderedDict(state)
    b1, b2, eps = 0.9, 0.999, 1e-8
    for k, g in grads.items():
        w = np.asarray(state[k], np.float64)
        g = np.asarray(g, np.float64) + hp["wd"] * w
        m, v = opt.get(k, (np.zeros_like(w), np.zeros_like(w)))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        opt[k] = (m, v)
        out[k] = w - hp["lr"] * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return out


def eval_features(state, x):
    """Eval-mode student features of spectrograms x [N, 1, 112, 112] (ndarray) -> [N, D]."""
    p = {k: torch.from_numpy(np.array(v)) for k, v in state.items()}
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
    with torch.no_grad():
        return encoder(p, "student", torch.from_numpy(np.asarray(x)).double(), False).numpy()
