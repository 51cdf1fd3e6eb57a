"""Float64 restatement, in plain torch on the CPU, of SpectrogramEncoderViT and of one
UniModalDINO + UniModalDINOLightning training step over it (models/dino.py:532-546, 1240-1398,
1596-1668; models/dino_vit.py:27-63, 122-177), written out from the formulas -- patch rows, one
GEMM, cls / position tokens, four post-norm layers (multi-head self-attention, residual +
LayerNorm, GELU MLP, residual + LayerNorm), the final LayerNorm, the cls row, Linear -- without
nn.TransformerEncoderLayer or nn.MultiheadAttention.  Dropout is off here, as in the fixtures.

tests/test_vit_cpu.py pins it to the reference's float64 fixtures (tests/golden/
uni_specvit_g2l2_f64.npz, made by tests/golden/gen_vit_golden.py) to 1e-8, so the GPU tests can
use it as the yardstick where the reference itself does not exist.

Parameters are a pure function of (seed, state-dict key) -- oracle.params.make_tensor -- so the
fixtures hold outputs only.  cls_token and pos_embed are non-zero, the attention biases too, and
in_proj_weight is scaled by ATTN_SCALE so that the attention is far from uniform (with torch's
initialisation the dQ / dK path carries gradients of 1e-5 and below, and a broken one would pass
every relative check).

Also here: a numpy restatement of csrc/common.h's hash_u32 / dropout_scale, for the kernels' masks.
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle.params import make_tensor
from tests.lstm_ref import adam_update, audio_views, dino_loss, head  # noqa: F401

KIND = "spectrogram_vit"
# the fixture case: D = 32, P = 16, B = 3, 2 global + 2 local views (12 student sequences), 3 steps
NAME = "uni_specvit_g2l2"
DIMS = dict(D=32, P=16, B=3, G=2, L=2)
PSEED, BSEED, STEPS = 811, 8110, 3
EVAL_NAME, EVAL_BATCHES, EVAL_SEED = "specvit_eval_features", (4, 3), 8200
HP = dict(lr=1e-4, wd=1e-6, momentum=0.996, center_momentum=0.9, tau_s=0.1, tau_t=0.04)
HW, PATCH, EMBED, DEPTH, HEADS = 112, 8, 512, 4, 4
LN_EPS = 1e-5
ATTN_SCALE = 3.0     # in_proj_weight = ATTN_SCALE * U(+-1/sqrt(E)); see gen_vit_golden's conditions
TOK_SCALE = 10.0     # cls_token, pos_embed = TOK_SCALE * U(+-0.1): tokens that differ by position

# avdino.spec kinds -> oracle.params kinds
_KIND = {"w": "dense_w", "b": "dense_b", "bn_w": "bn_w", "bn_b": "bn_b", "rm": "rm", "rv": "rv",
         "nbt": "nbt", "center": "center", "tok": "dense_b", "attn_w": "dense_w", "attn_b": "dense_b",
         "ln_w": "bn_w", "ln_b": "bn_b"}
PARAM_KINDS = ("w", "b", "bn_w", "bn_b", "tok", "attn_w", "attn_b", "ln_w", "ln_b")


def vit_spec(D, P):
    from avdino.spec import unimodal_dino_sd
    return unimodal_dino_sd(KIND, D, P)


def vit_state(spec, seed, stats=False):
    """key -> ndarray.  stats: running statistics away from (0, 1), for the eval-mode fixture."""
    out = OrderedDict()
    for k, (shp, kind) in spec.items():
        okind = _KIND[kind]
        if stats and kind in ("rm", "rv"):
            okind = "bn_b" if kind == "rm" else "bn_w"
        v = make_tensor(seed, k, shp, okind)
        if kind == "attn_w":
            v = (v * np.float32(ATTN_SCALE)).astype(np.float32)
        elif kind == "tok":
            v = (v * np.float32(TOK_SCALE)).astype(np.float32)
        out[k] = v
    return out


def layer_norm(x, g, b):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS) * g + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(x, w_in, b_in, heads, probs=None):
    """softmax(q k^T / sqrt(dh)) v per head on x [N, T, E]; probs: list to append the mean over
    (sequence, head, query) of the largest probability to."""
    N, T, E = x.shape
    dh = E // heads
    qkv = x @ w_in.T + b_in
    q, k, v = (t.reshape(N, T, heads, dh).permute(0, 2, 1, 3) for t in qkv.split(E, dim=-1))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    s = s - s.max(dim=-1, keepdim=True).values
    e = torch.exp(s)
    pr = e / e.sum(dim=-1, keepdim=True)
    if probs is not None:
        probs.append(float(pr.detach().max(dim=-1).values.mean()))
    return (pr @ v).permute(0, 2, 1, 3).reshape(N, T, E)


def patch_rows(x, patch):
    """x [N, 1, H, W] -> [N, (H/p)(W/p), p*p], rows in (gy, gx) order, features in (ph, pw)."""
    N, _c, H, W = x.shape
    gh, gw = H // patch, W // patch
    return x.reshape(N, gh, patch, gw, patch).permute(0, 1, 3, 2, 4).reshape(N, gh * gw, patch * patch)


def tower(p, e, x, heads=HEADS, patch=PATCH, probs=None):
    """AudioViTEncoder under the key prefix ``e`` ("....encoder.0.") on x [N, 1, H, W] -> the
    normalised cls row [N, E]."""
    w = p[e + "patch_embed.projection.weight"]
    E = w.shape[0]
    pe = patch_rows(x, patch) @ w.reshape(E, -1).T + p[e + "patch_embed.projection.bias"]
    N = x.shape[0]
    h = torch.cat([p[e + "cls_token"].expand(N, 1, E), pe], dim=1) + p[e + "pos_embed"]
    i = 0
    while f"{e}transformer.layers.{i}.linear1.weight" in p:
        l = f"{e}transformer.layers.{i}."
        a = attention(h, p[l + "self_attn.in_proj_weight"], p[l + "self_attn.in_proj_bias"], heads, probs)
        a = a @ p[l + "self_attn.out_proj.weight"].T + p[l + "self_attn.out_proj.bias"]
        h = layer_norm(h + a, p[l + "norm1.weight"], p[l + "norm1.bias"])
        f = gelu(h @ p[l + "linear1.weight"].T + p[l + "linear1.bias"])
        f = f @ p[l + "linear2.weight"].T + p[l + "linear2.bias"]
        h = layer_norm(h + f, p[l + "norm2.weight"], p[l + "norm2.bias"])
        i += 1
    h = layer_norm(h, p[e + "transformer.norm.weight"], p[e + "transformer.norm.bias"])
    return h[:, 0]


def encoder(p, prefix, x, probs=None):
    """One call of SpectrogramEncoderViT on x [B, 1, 112, 112]; p: key -> float64 tensor."""
    c = tower(p, prefix + ".encoder.0.", x, probs=probs)
    return c @ p[prefix + ".encoder.1.weight"].T + p[prefix + ".encoder.1.bias"]


# Student gradients that are mathematically zero (1e-14 and below in float64), so they have no
# relative error:
#   - the k third of every in_proj_bias: a constant added to every key's score leaves the softmax
#     unchanged;
#   - the final LayerNorm's bias, the Linear(512, D) bias behind it and the projection head's mlp.0
#     bias: each adds the same vector to every row of a train-mode BatchNorm1d's input (through
#     linear maps), which the batch statistics remove.
ZERO_K_BIAS = tuple(f"student.encoder.0.transformer.layers.{i}.self_attn.in_proj_bias" for i in range(DEPTH))
ZERO_BN_BIAS = ("student.encoder.0.transformer.norm.bias", "student.encoder.1.bias",
                "student_projection.mlp.0.bias")


def grad_slices(k, g):
    """[(suffix, array)] a gradient is compared by: the q / k / v thirds of an attention
    in-projection ("#q", "#k", "#v"), else the whole tensor ("")."""
    if "in_proj_" in k:
        E = g.shape[0] // 3
        return [("#" + n, g[i * E:(i + 1) * E]) for i, n in enumerate("qkv")]
    return [("", g)]


def is_zero_grad(k, sfx):
    return (k in ZERO_K_BIAS and sfx == "#k") or k in ZERO_BN_BIAS


def _is_param(spec, k):
    return spec[k][1] in PARAM_KINDS


def unimodal_step(state, batch, hp, spec, probs=None):
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
    emb = torch.cat([encoder(p, "student", x[v], probs) for v in range(V)])
    with torch.no_grad():
        temb = torch.cat([encoder(p, "teacher", x[v]) for v in range(G)])
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
        if k.endswith("num_batches_tracked"):     # only the projection heads have BatchNorm: once each
            new[k] = new[k] + 1
    return dict(loss=float(loss.item()), s_out=s_out.detach().numpy(), t_out=t_out.numpy(),
                emb=emb.detach().view(V, B, -1).numpy(), grads=grads, state=new,
                center_after=center_after.numpy())


def eval_features(state, x):
    """Eval-mode student features of spectrograms x [N, 1, 112, 112] (ndarray) -> [N, D]."""
    p = {k: torch.from_numpy(np.array(v)) for k, v in state.items()}
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
    with torch.no_grad():
        return encoder(p, "student", torch.from_numpy(np.asarray(x)).double()).numpy()


# ---------------------------------------------------------------- the kernels' dropout masks
_M64 = (1 << 64) - 1


def hash_u32(seed, idx):
    """csrc/common.h hash_u32 on integer arrays (uint64 arithmetic modulo 2^64)."""
    with np.errstate(over="ignore"):
        seed = np.asarray(seed, np.uint64)
        idx = np.asarray(idx, np.uint64)
        x = (seed * np.uint64(0x9E3779B97F4A7C15)) ^ (idx + np.uint64(0xD1B54A32D192ED03))
        x ^= x >> np.uint64(33)
        x = x * np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x = x * np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def dropout_scale(seed, idx, p):
    """csrc/common.h dropout_scale: float64 array of 0 or the f32 value 1/(1-p)."""
    idx = np.asarray(idx, np.uint64)
    if p <= 0:
        return np.ones(idx.shape, np.float64)
    u = (hash_u32(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(u >= np.float32(p), np.float64(keep), 0.0)
