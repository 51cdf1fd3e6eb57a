"""The audio ViT encoder (spectrogram_vit) without a GPU: the float64 restatement tests/vit_ref.py
is pinned to the reference's float64 fixtures, and the spec, initialisation, checkpoint,
command-line and argument-validation surface of the new encoder -- with the fences other tests
set (spec.UNI_ENCODERS stays the four conv-stack kinds; submit_models does not know the kind yet)
visible here too."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle.params import make_multimodal_batch
from tests import golden_util as gu
from tests import vit_ref as VR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(REPO, "configs", "config_multimodal_dino.yaml")
D, P, B, G, L = (VR.DIMS[k] for k in "DPBGL")
PREFIX = "student.encoder.0."


def _check(fx, key, value, rel=1e-8):
    ok, msg = gu.compare(fx, key, value, rel=rel)
    assert ok, msg


def _ref_keys():
    return json.load(open(os.path.join(gu.GOLDEN, "vit_state_keys.json")))[f"spectrogram_vit/D{D}_P{P}"]


@pytest.fixture(scope="module")
def ref_step():
    spec = VR.vit_spec(D, P)
    state = VR.vit_state(spec, VR.PSEED)
    batch = make_multimodal_batch(B, G, L, VR.BSEED, with_originals=False)
    probs = []
    return spec, state, VR.unimodal_step(state, batch, VR.HP, spec, probs=probs), probs


def test_vit_ref_reproduces_the_float64_fixture(ref_step):
    spec, state, r, probs = ref_step
    fx = gu.load(VR.NAME + "_f64")
    assert abs(r["loss"] - float(fx["loss"])) < 1e-8
    _check(fx, "s_out", r["s_out"])
    _check(fx, "t_out", r["t_out"])
    _check(fx, "emb", r["emb"])
    assert sorted(r["grads"]) == sorted(str(k) for k in fx["live_keys"])
    seen_zero = set()
    for k, g in r["grads"].items():
        for sfx, a in VR.grad_slices(k, g):
            if VR.is_zero_grad(k, sfx):
                assert np.linalg.norm(a) < 1e-12, (k, sfx)
                seen_zero.add(k)
            else:
                assert np.linalg.norm(a) >= 1e-4, (k, sfx)      # the generator's second condition
                _check(fx, "grad/" + k + sfx, a)
    assert seen_zero == set(VR.ZERO_K_BIAS) | set(VR.ZERO_BN_BIAS)
    # the generator's first condition: the attention is neither uniform nor one-hot in any layer
    per_layer = np.array(probs).reshape(-1, VR.DEPTH).mean(axis=0)
    assert all(0.05 <= v <= 0.9 for v in per_layer), per_layer
    np.testing.assert_allclose(r["center_after"], fx["center_after"], atol=1e-10, rtol=0)
    new = r["state"]
    for k in spec:
        if k.endswith("running_mean") or k.endswith("running_var"):
            _check(fx, "rs/" + k, new[k])
        elif k.startswith("teacher") and not k.endswith("num_batches_tracked"):
            _check(fx, "ema/" + k, new[k])
    post = VR.adam_update(new, r["grads"], {}, 1, VR.HP)
    for k in r["grads"]:
        _check(fx, "post/" + k, post[k])


def test_vit_ref_loss_curve_and_eval_features():
    spec = VR.vit_spec(D, P)
    st = VR.vit_state(spec, VR.PSEED)
    opt, curve = {}, []
    for step in range(VR.STEPS):
        b = make_multimodal_batch(B, G, L, VR.BSEED + step, with_originals=False)
        r = VR.unimodal_step(st, b, VR.HP, spec)
        curve.append(r["loss"])
        st = VR.adam_update(r["state"], r["grads"], opt, step + 1, VR.HP)
    np.testing.assert_allclose(curve, gu.load(VR.NAME + "_f64")["curve"], atol=1e-8, rtol=0)
    fx = gu.load(VR.EVAL_NAME + "_f64")
    assert tuple(fx["meta_batches"]) == VR.EVAL_BATCHES
    state = VR.vit_state(spec, VR.PSEED, stats=True)
    for i, n in enumerate(VR.EVAL_BATCHES):
        x = make_multimodal_batch(n, 1, 1, VR.EVAL_SEED + i)["audio"]
        f = VR.eval_features(state, x)
        assert f.shape == (n, D)
        assert gu.rel_err(f, fx[f"feat{i}"]) < 1e-8


def test_fixture_parameters_are_not_the_zero_initialisation():
    st = VR.vit_state(VR.vit_spec(D, P), VR.PSEED)
    for k in ("cls_token", "pos_embed", "transformer.layers.0.self_attn.in_proj_bias",
              "transformer.layers.3.self_attn.out_proj.bias", "transformer.norm.bias"):
        assert float(np.abs(st[PREFIX + k]).max()) > 0.05, k


def test_state_dict_keys_order_and_shapes():
    from avdino import spec as S
    from avdino.models import SpectrogramEncoderViT, UniModalDINO
    ref = _ref_keys()
    spec = VR.vit_spec(D, P)
    assert [[k, list(shp)] for k, (shp, _kind) in spec.items()] == ref
    m = UniModalDINO(encoder_class=SpectrogramEncoderViT, output_dim=D, projection_dim=P, device="cpu")
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref
    keys = [k for k, _ in ref]
    # nn.Parameters of the encoder module precede its submodules' keys
    assert keys[1:3] == [PREFIX + "cls_token", PREFIX + "pos_embed"]
    assert spec[PREFIX + "pos_embed"][0] == (1, 197, 512)
    assert (S.VIT_AUDIO["patch"], S.VIT_AUDIO["embed_dim"], S.VIT_AUDIO["depth"], S.VIT_AUDIO["heads"],
            S.VIT_MLP_RATIO * S.VIT_AUDIO["embed_dim"], S.VIT_LN_EPS) == (8, 512, 4, 4, 2048, 1e-5)


def test_fences_conv_stack_table_and_submit_models():
    from avdino import spec as S
    from avdino import submit_models as SM
    assert len(S.UNI_ENCODERS) == 4 and "spectrogram_vit" not in S.UNI_ENCODERS
    assert all(isinstance(e[1]("s"), S.ConvStackSpec) for e in S.UNI_ENCODERS.values())
    assert list(S.VIT_ENCODERS) == ["spectrogram_vit"]
    assert S.uni_kinds() == tuple(S.UNI_ENCODERS) + ("spectrogram_vit",)
    assert S.uni_modality("spectrogram_vit") == "audio" and S.uni_modality("image") == "image"
    with pytest.raises(SystemExit):
        SM.main(["--models", "spectrogram_vit", "--config", CFG, "--dry-run"])


def test_initialisation_per_kind():
    from avdino.params import ParamStore
    store = ParamStore(VR.vit_spec(D, P), "cpu", seed=3)
    E = 512
    l = PREFIX + "transformer.layers.2."
    w = store[l + "self_attn.in_proj_weight"]
    xav = math.sqrt(6.0 / (3 * E + E))                       # xavier_uniform_ on [3E, E]
    assert w.shape == (3 * E, E) and 0.99 * xav < float(w.abs().max()) <= xav
    assert float(w.std()) == pytest.approx(xav / math.sqrt(3), rel=0.02)
    for k in (l + "self_attn.in_proj_bias", l + "self_attn.out_proj.bias", PREFIX + "cls_token",
              PREFIX + "pos_embed", l + "norm1.bias", l + "norm2.bias", PREFIX + "transformer.norm.bias"):
        assert float(store[k].abs().max()) == 0.0, k
    for k in (l + "norm1.weight", l + "norm2.weight", PREFIX + "transformer.norm.weight"):
        assert torch.equal(store[k], torch.ones(E)), k
    for k, fan in ((l + "self_attn.out_proj", E), (l + "linear1", E), (l + "linear2", 4 * E),
                   (PREFIX + "patch_embed.projection", 64), ("student.encoder.1", E)):
        b = 1.0 / math.sqrt(fan)                             # Linear / Conv2d defaults
        for t in (store[k + ".weight"], ) + (() if "out_proj" in k else (store[k + ".bias"], )):
            assert float(t.abs().max()) <= b, k
            assert t.numel() < 256 or float(t.abs().max()) > 0.9 * b, k
    for k in store.t_offs:
        assert torch.equal(store[k], store["student" + k[len("teacher"):]]), k


def test_model_map_cli_and_checkpoint_round_trip(tmp_path):
    from avdino import models as M
    from avdino import run_dino as R
    from avdino.trainer import load_checkpoint, save_checkpoint
    enc = M.SpectrogramEncoderViT
    assert M.UNIMODAL_MODEL_MAP["spectrogram_vit"] is enc
    assert enc.modality == "audio" and enc(64).output_dim == 64 and enc.kind == "spectrogram_vit"
    cfg = R.load_config(CFG)
    a = R.parse_args(["--unimodal_model", "spectrogram_vit", "--config", CFG, "--precision", "32"])
    m = R.build_model(a, cfg, device="cpu")
    assert type(m) is M.UniModalDINOLightning and type(m.model.student_spec) is enc
    for name in ("multi_vit", "multi_dual_vit"):             # stay rejected everywhere
        assert name not in M.MODEL_MAP and name not in M.UNIMODAL_MODEL_MAP
        with pytest.raises(SystemExit):
            R.parse_args(["--model", name, "--config", CFG])
    m = M.UniModalDINOLightning(encoder_class=enc, output_dim=D, projection_dim=P, device="cpu")
    spec = VR.vit_spec(D, P)
    m.load_state_dict({"model." + k: torch.from_numpy(np.array(v)) for k, v in VR.vit_state(spec, 5).items()})
    path = str(tmp_path / "x.ckpt")
    save_checkpoint(m, path, epoch=3, global_step=12)
    assert load_checkpoint(path)["hyper_parameters"]["encoder_class"] == enc.__name__
    m2 = M.UniModalDINOLightning.load_from_checkpoint(path, device="cpu")
    assert type(m2.model.student_spec) is enc
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    bad = dict(m.state_dict())
    bad.pop("model.teacher.encoder.0.pos_embed")
    with pytest.raises(RuntimeError, match="Missing"):
        m2.load_state_dict(bad)


def test_model_stats_parameters_and_macs():
    from avdino import models as M
    from avdino import run_dino as R
    nparam = sum(int(np.prod(shp)) for k, shp in _ref_keys()
                 if not k.endswith(("running_mean", "running_var", "num_batches_tracked")) and k != "center")
    m = M.UniModalDINOLightning(encoder_class=M.SpectrogramEncoderViT, output_dim=D, projection_dim=P,
                                device="cpu")
    gflops, params = R.model_stats(m, 2, 4)
    assert params == nparam
    E, Tp, T, F = 512, 196, 197, 2048
    enc = Tp * 64 * E + 4 * (T * (3 * E * E + E * E + 2 * E * F) + 2 * 4 * T * T * 128) + E * D
    head = D * 512 + 512 * P
    assert gflops == pytest.approx((6 + 2) * (enc + head) / 1e9, rel=1e-12)


def test_hyper_keeps_its_defaults_and_gains_vit_dropout():
    from avdino.engine import Hyper
    h = Hyper()
    assert (h.vit_dropout, h.dropout, h.fusion_dropout, h.lr, h.wd) == (0.1, 0.3, 0.3, 1e-4, 1e-6)
    assert Hyper(vit_dropout=0.0).vit_dropout == 0.0


def test_site_seeds_never_collide():
    from avdino import vit
    seeds = {vit.site_seed(b, r, i, s) + 16 * t for b in (0, 12345, (1 << 48) - 1) for r in (0, 1)
             for i in range(4) for s in vit.SITES for t in (0, 1, 1000)}
    assert len(seeds) == 3 * 2 * 4 * 4 * 3
    assert all(s >> 48 >= 1 for s in seeds)                  # site 0 is the engine's other dropouts


def test_numpy_hash_matches_common_h_on_literals():
    """hash_u32 of csrc/common.h, evaluated by hand (Python integers modulo 2^64) from its
    formula, against the numpy restatement; and dropout_scale's threshold and scale."""
    def by_hand(seed, idx):
        M = (1 << 64) - 1
        x = ((seed * 0x9E3779B97F4A7C15) & M) ^ ((idx + 0xD1B54A32D192ED03) & M)
        x ^= x >> 33
        x = (x * 0xff51afd7ed558ccd) & M
        x ^= x >> 33
        x = (x * 0xc4ceb9fe1a85ec53) & M
        x ^= x >> 33
        return x & 0xFFFFFFFF

    literals = {(0, 0): 0xf1592379, (1, 0): 0x18923fd1, (7, 123456789): 0x4888d2b5,
                ((1 << 63) + 5, (1 << 40) + 3): 0xd32f6c4f, (3, 2 ** 33): 0x385a0be6}
    for (seed, idx), want in literals.items():
        assert by_hand(seed, idx) == want, (seed, idx)
        assert int(VR.hash_u32(seed, idx)) == want, (seed, idx)
    seeds = np.array([3, 3, 99], np.uint64)
    idx = np.array([0, 1, 2 ** 33], np.uint64)
    assert [int(v) for v in VR.hash_u32(seeds, idx)] == [by_hand(3, 0), by_hand(3, 1), by_hand(99, 2 ** 33)]
    idx = np.arange(1 << 16, dtype=np.uint64)
    m = VR.dropout_scale(5, idx, 0.25)
    u = (VR.hash_u32(5, idx) >> np.uint32(8)).astype(np.float64) / 16777216.0
    assert np.array_equal(m > 0, u >= np.float32(0.25))
    assert set(np.unique(m)) == {0.0, float(np.float32(1.0) / np.float32(0.75))}
    assert abs((m > 0).mean() - 0.75) < 0.01
    assert np.array_equal(VR.dropout_scale(5, idx, 0.0), np.ones(idx.shape))


def test_vit_argument_validation_without_launch():
    from avdino._lib import lib
    d = ctypes.c_void_p(4096)

    def fwd(q=d, ctx=d, ld=512, N=2, heads=4, T=197, dh=128, dt=0, p=0.0):
        return lib.avd_mhsa_fwd(q, ld, d, ld, d, ld, ctx, ld, None, N, heads, T, dh, dt, 0.1, p, 0, None, None)

    for kw in (dict(dh=16), dict(dh=96), dict(dh=256), dict(T=0), dict(T=257), dict(N=0), dict(heads=0)):
        assert fwd(**kw) == -1, kw
    assert fwd(dt=2) == -2
    for kw in (dict(q=None), dict(ctx=None), dict(ld=508), dict(ld=514), dict(q=ctypes.c_void_p(4100)),
               dict(p=1.0), dict(p=-0.1)):
        assert fwd(**kw) == -4, kw
    assert lib.avd_mhsa_bwd_ws(3, 4, 197, 128) == 3 * (3 * 4 * 197)     # corr, delta hi, delta lo per row
    assert lib.avd_mhsa_bwd_ws(3, 4, 300, 128) == -1 and lib.avd_mhsa_bwd_ws(3, 4, 197, 48) == -1

    def bwd(dout=d, ws=d, nws=1 << 20, ld=512, T=50, dh=128, dt=1):
        return lib.avd_mhsa_bwd(dout, ld, d, ld, d, ld, d, ld, d, d, ld, d, ld, d, ld, ws, nws, 2, 4, T, dh,
                                dt, 0.1, 0.0, 0, None, None)

    assert bwd(T=300) == -1 and bwd(dh=8) == -1 and bwd(dt=5) == -2
    assert bwd(dout=None) == -4 and bwd(ws=None) == -4 and bwd(nws=10) == -4 and bwd(ld=510) == -4

    def ln(x=d, y=d, rows=7, E=512, ld=512, p=0.0):
        return lib.avd_ln_fwd(x, ld, None, ld, d, d, y, ld, None, None, None, rows, E, 1e-5, p, 0, None, None)

    assert ln(E=16) == -1 and ln(E=48) == -1 and ln(E=544) == -1 and ln(rows=0) == -1
    assert ln(x=None) == -4 and ln(y=None) == -4 and ln(ld=256) == -4 and ln(p=1.5) == -4
    assert lib.avd_ln_bwd_ws(300, 512) == 10 * 2 * 512 and lib.avd_ln_bwd_ws(300, 40) == -1
    assert lib.avd_gelu_fwd(d, d, 0, 8, 0.0, 0, None, None) == -1
    assert lib.avd_gelu_fwd(None, d, 4, 8, 0.0, 0, None, None) == -4
    assert lib.avd_gelu_bwd(d, d, None, 4, 8, 0.0, 0, None, None) == -4
    assert lib.avd_vit_patchify(d, 0, d, 2, 112, 112, 9, None) == -1
    assert lib.avd_vit_patchify(d, 3, d, 2, 112, 112, 8, None) == -2
    assert lib.avd_vit_patchify(None, 0, d, 2, 112, 112, 8, None) == -4
    assert lib.avd_vit_tokens_fwd(d, d, d, d, 2, 1, 512, None) == -1
    assert lib.avd_vit_tokens_bwd(d, None, 2, 197, 512, None) == -4


def test_ops_vit_wrappers_check_sizes_on_the_host():
    """ops.mhsa_* / ln_* reject operands the kernel would read or write out of bounds before any
    launch (CPU tensors: a launch would fail differently)."""
    from avdino import ops
    N, heads, T, dh = 2, 2, 5, 32
    E, R = heads * dh, N * T
    qkv, ctx, lse = torch.zeros(R * 3 * E), torch.zeros(R * E), torch.zeros(N * heads * T)
    q, k, v = (qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E)
    with pytest.raises(ValueError, match="one of"):
        ops.mhsa_fwd(q, k, v, (ctx, 0, E), lse, N, 1, T, 48, 0.1, False)
    with pytest.raises(ValueError, match="T <= 256"):
        ops.mhsa_fwd(q, k, v, (ctx, 0, E), lse, N, heads, 257, dh, 0.1, False)
    with pytest.raises(ValueError, match="v bounds"):
        ops.mhsa_fwd(q, k, (qkv[:-1], 2 * E, 3 * E), (ctx, 0, E), lse, N, heads, T, dh, 0.1, False)
    with pytest.raises(ValueError, match="ctx bounds"):
        ops.mhsa_fwd(q, k, v, (ctx[:-1], 0, E), lse, N, heads, T, dh, 0.1, False)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.mhsa_fwd(q, (qkv, E + 2, 3 * E), v, (ctx, 0, E), lse, N, heads, T, dh, 0.1, False)
    with pytest.raises(ValueError, match="lse"):
        ops.mhsa_fwd(q, k, v, (ctx, 0, E), lse[:-1], N, heads, T, dh, 0.1, False)
    with pytest.raises(ValueError, match="dropout"):
        ops.mhsa_fwd(q, k, v, (ctx, 0, E), lse, N, heads, T, dh, 0.1, False, drop_p=1.0)
    with pytest.raises(ValueError, match="workspace"):
        ops.mhsa_bwd((ctx, 0, E), q, k, v, lse, q, k, v, torch.zeros(3), N, heads, T, dh, 0.1, False)
    x, g = torch.zeros(7 * 64), torch.zeros(64)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.ln_fwd(x, None, g, g, x, 7, 48)
    with pytest.raises(ValueError, match="x bounds"):
        ops.ln_fwd(x, None, g, g, x, 7, 64, x_ld=65)
    with pytest.raises(ValueError, match="y bounds"):
        ops.ln_fwd(x, None, g, g, x[:-1], 7, 64)
    with pytest.raises(ValueError, match="workspace"):
        ops.ln_bwd(x, x, g, g, g, x, None, g, g, torch.zeros(3), 7, 64)
    with pytest.raises(ValueError, match="gelu"):
        ops.gelu_fwd(x, x[:-1], 7, 64)
    with pytest.raises(ValueError, match="patchify"):
        ops.vit_patchify(torch.zeros(2 * 16 * 16), torch.zeros(2 * 16 * 16), 2, 16, 16, 5)
    with pytest.raises(ValueError, match="tokens"):
        ops.vit_tokens_fwd(torch.zeros(2 * 4 * 32), torch.zeros(32), torch.zeros(4 * 32), torch.zeros(2 * 5 * 32),
                           2, 5, 32)
    from avdino.vit import ViTTower
    with pytest.raises(ValueError, match="embed_dim / heads"):
        ViTTower("s", 112, 8, 512, 4, 2, torch.float32, ops.GEMM_F32_MFMA)
    with pytest.raises(ValueError, match="tokens"):
        ViTTower("s", 112, 4, 512, 4, 4, torch.float32, ops.GEMM_F32_MFMA)
    t = ViTTower("s", 112, 8, 512, 4, 4, torch.float32, ops.GEMM_F32_MFMA)
    R = 768 * 197
    # the issue's figure: one saved FF activation is R * 2048 * 4 bytes = 1.24 GB at B = 128
    assert R * 2048 * 4 == pytest.approx(1.24e9, rel=0.01)
    assert t.activation_elems(768, True) > 4 * R * 16 * 512 and t.activation_elems(768, False) < R * 24 * 512
