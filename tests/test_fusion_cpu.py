"""The gated and cross-attention fusion encoders on CPU (no engine, no launch): reference
state-dict keys and their order, parameter initialisation, .ckpt round trip, MODEL_MAP /
run_dino / submit_models surface, and the new entry points' argument validation."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import fusion_util as FU

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(REPO, "configs", "config_multimodal_dino.yaml")
KEYS = json.load(open(os.path.join(REPO, "tests", "golden", "fusion_state_keys.json")))
MODES = ("default", "mse", "infonce", "semi_supervised")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("encoder", list(FU.ENCODERS))
def test_state_dict_keys_and_order_are_the_references(encoder, mode):
    from avdino import models as M
    cls = M.MULTIMODAL_WRAPPERS[mode]
    m = cls(encoder_class=M.MODEL_MAP[encoder], encoder_output_dim=32, output_dim=32, projection_dim=16,
            device="cpu")
    ref = KEYS[f"{encoder}/{mode}"]
    assert list(m.model.state_dict().keys()) == ref
    assert list(m.state_dict().keys()) == ["model." + k for k in ref]
    sd = m.model.state_dict()
    if encoder == "multi_simple_gated":
        assert ref[1:3] == ["student.gate_image", "student.gate_audio"]          # before the towers
        assert sd["student.gate_image"].shape == () and float(sd["teacher.gate_audio"]) == 0.5
    else:
        i = ref.index("student.fusion.3.bias")
        assert ref[i + 1:i + 9] == [f"student.{a}.{p}.{w}" for a in ("image_to_audio_attention",
                                                                     "audio_to_image_attention")
                                    for p in ("q_proj", "kv_proj") for w in ("weight", "bias")]
        assert sd["student.image_to_audio_attention.q_proj.weight"].shape == (32, 32)
        assert sd["student.audio_to_image_attention.kv_proj.weight"].shape == (64, 32)
        assert sd["student.audio_to_image_attention.kv_proj.bias"].shape == (64,)


def test_new_parameters_are_trainable_ema_and_default_initialised():
    from avdino.params import ParamStore
    for encoder, keys in (("multi_simple_gated", ["student.gate_image", "student.gate_audio"]),
                          ("multi_cross_attention", ["student.image_to_audio_attention.q_proj.weight",
                                                     "student.audio_to_image_attention.kv_proj.bias"])):
        st = ParamStore(FU.fusion_spec("mse", 32, 32, 16, encoder), "cpu", seed=3)
        for k in keys:
            assert k in st.live_keys                                   # gradient arena: Adam, DDP
            tk = "teacher." + k[len("student."):]
            assert tk in st.t_offs and torch.equal(st[k], st[tk])      # EMA'd into the teacher
            assert st.s_offs[k][0] - st.n_heads == st.t_offs[tk][0]
        if encoder == "multi_simple_gated":
            assert float(st["student.gate_image"]) == 0.5 and float(st["student.gate_audio"]) == 0.5
        else:
            w = st["student.image_to_audio_attention.kv_proj.weight"]
            b = 1.0 / np.sqrt(32)                                       # nn.Linear default: U(+-1/sqrt(fan_in))
            assert float(w.abs().max()) <= b and float(w.abs().max()) > 0.9 * b and abs(float(w.mean())) < 0.02


@pytest.mark.parametrize("encoder", list(FU.ENCODERS))
def test_checkpoint_round_trip(encoder, tmp_path):
    from avdino import models as M
    from avdino.trainer import load_checkpoint, save_checkpoint
    enc = M.MODEL_MAP[encoder]
    m = M.MultiModalDINOWithMSELightning(encoder_class=enc, encoder_output_dim=32, output_dim=32,
                                         projection_dim=16, device="cpu", learning_rate=3e-4, num_epochs=7)
    spec = FU.fusion_spec("mse", 32, 32, 16, encoder)
    m.load_state_dict({"model." + k: torch.from_numpy(np.array(v)) for k, v in FU.fusion_state(spec, 5).items()})
    path = str(tmp_path / "x.ckpt")
    save_checkpoint(m, path, epoch=3, global_step=12)
    assert load_checkpoint(path)["hyper_parameters"]["encoder_class"] == enc.__name__
    m2 = M.MultiModalDINOWithMSELightning.load_from_checkpoint(path, device="cpu")
    assert type(m2.model.student_spec) is enc
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    if encoder == "multi_simple_gated":
        assert float(m2.state_dict()["model.student.gate_image"]) == pytest.approx(FU.GATES["gate_image"])
    bad = dict(m.state_dict())
    bad.pop("model.student.gate_audio" if encoder == "multi_simple_gated"
            else "model.teacher.audio_to_image_attention.q_proj.bias")
    with pytest.raises(RuntimeError, match="Missing"):
        m2.load_state_dict(bad)


def test_model_map_and_reference_signatures():
    import inspect

    from avdino import models as M
    assert M.MODEL_MAP["multi_simple_gated"] is M.GatedMultiModalEncoder
    assert M.MODEL_MAP["multi_cross_attention"] is M.CrossAttentionMultiModalEncoder
    assert list(inspect.signature(M.GatedMultiModalEncoder.__init__).parameters) == \
        ["self", "output_dim", "encoder_output_dim"]
    assert list(inspect.signature(M.CrossAttentionMultiModalEncoder.__init__).parameters) == \
        ["self", "output_dim", "encoder_output_dim", "fusion_dropout"]
    e = M.CrossAttentionMultiModalEncoder(64, 128, 0.1)
    assert e.fusion_dropout == 0.1 and e.image_to_audio_attention.dim == 128
    assert e.audio_to_image_attention.scale == 128 ** -0.5
    assert M.GatedMultiModalEncoder(64, 128).fusion_dropout == 0.3
    # an unsupported encoder_output_dim is refused at construction, with the supported list
    with pytest.raises(ValueError, match=r"\(32, 64, 128, 256, 512\)"):
        M.MultiModalDINOWithMSE(encoder_class=M.CrossAttentionMultiModalEncoder, encoder_output_dim=48,
                                output_dim=32, projection_dim=16, device="cpu")
    # the gated encoder has no such limit
    M.MultiModalDINOWithMSE(encoder_class=M.GatedMultiModalEncoder, encoder_output_dim=48, output_dim=32,
                            projection_dim=16, device="cpu")


def test_run_dino_and_submit_models_accept_the_new_names(capsys):
    from avdino import run_dino as R
    from avdino import submit_models as SM
    cfg = R.load_config(CFG)
    for name, cls in (("multi_cross_attention", "CrossAttentionMultiModalEncoder"),
                      ("multi_simple_gated", "GatedMultiModalEncoder")):
        a = R.parse_args(["--model", name, "--training_mode", "mse", "--config", CFG, "--precision", "32"])
        m = R.build_model(a, cfg, device="cpu")
        assert type(m).__name__ == "MultiModalDINOWithMSELightning"
        assert type(m.model.student_spec).__name__ == cls
    cmds = SM.main(["--models", "multi_simple_gated", "multi_cross_attention", "--training_mode", "mse",
                    "--config", CFG, "--dry-run"])
    assert len(cmds) == 2 and capsys.readouterr().out.count("Submitting:") == 2
    assert cmds[0][1:] == ["-m", "avdino.run_dino", "--model", "multi_simple_gated", "--config", CFG,
                           "--metric", "mlp_acc", "--training_mode", "mse"]
    assert cmds[1][4] == "multi_cross_attention"
    with pytest.raises(SystemExit):
        SM.main(["--models", "multi_lstm", "--config", CFG, "--dry-run"])


def test_model_stats_count_the_new_parameters_and_attention_flops():
    from avdino import models as M
    from avdino import run_dino as R
    E, D, P = 64, 32, 16

    def stats(enc, B=1):
        m = M.MultiModalDINOWithMSELightning(encoder_class=enc, encoder_output_dim=E, output_dim=D,
                                             projection_dim=P, device="cpu")
        return R.model_stats(m, 2, 4, B)

    g0, p0 = stats(M.SimpleMultiModalEncoder)
    gg, pg = stats(M.GatedMultiModalEncoder)
    gx, px = stats(M.CrossAttentionMultiModalEncoder, 1)
    gx8, _ = stats(M.CrossAttentionMultiModalEncoder, 9)
    assert pg == p0 + 2 * 2 and gg == g0                          # two gates, student and teacher
    att = 2 * (E * E + E + 2 * E * E + 2 * E)                     # q_proj + kv_proj, both directions
    assert px == p0 + 2 * att
    per_call = 2 * (E * E + 2 * E * E)                            # projection multiply-adds per sample
    assert gx == pytest.approx(g0 + (6 + 2) * (per_call + 4 * 1 * E) / 1e9, rel=1e-12)
    assert gx8 == pytest.approx(gx + (6 + 2) * 4 * 8 * E / 1e9, rel=1e-12)


def test_argument_validation_without_launch():
    from avdino._lib import lib
    d = ctypes.c_void_p(4096)
    E, B = 64, 5

    def fwd(q=d, out=d, ldq=3 * E, dsq=0, ldo=2 * E, dirs=1, groups=2, B=B, E=E):
        return lib.avd_xattn_fwd(q, ldq, dsq, d, 3 * E, 0, d, 3 * E, 0, d, 2 * E, 0, out, ldo, 0, None,
                                 dirs, groups, B, E, 0.125, None)

    assert fwd(q=None) == -4 and fwd(out=None) == -4
    assert fwd(E=48) == -1 and fwd(E=1024) == -1 and fwd(B=0) == -1 and fwd(groups=0) == -1
    assert fwd(dirs=3) == -1 and fwd(ldq=E - 4) == -1 and fwd(ldo=E - 4) == -1
    assert fwd(ldq=3 * E + 2) == -4 and fwd(dsq=6) == -4            # whole float4s only
    assert fwd(q=ctypes.c_void_p(4100)) == -4                       # 16-byte aligned operands

    def bwd(dout=d, ws=d, ws_elems=2 * B, lddq=3 * E, E=E, B=B):
        return lib.avd_xattn_bwd(dout, 2 * E, 0, d, 3 * E, 0, d, 3 * E, 0, d, 3 * E, 0, d, d, lddq, 0,
                                 d, 3 * E, 0, d, 3 * E, 0, ws, ws_elems, 1, 2, B, E, 0.125, None)

    assert lib.avd_xattn_bwd_ws(1, 2, B, E) == 2 * B and lib.avd_xattn_bwd_ws(2, 3, 7, 32) == 42
    assert lib.avd_xattn_bwd_ws(1, 2, B, 48) == -1 and lib.avd_xattn_bwd_ws(1, 2, 0, E) == -1
    assert bwd(dout=None) == -4 and bwd(ws=None) == -4 and bwd(ws_elems=2 * B - 1) == -4
    assert bwd(E=96) == -1 and bwd(B=0) == -1 and bwd(lddq=E - 4) == -1

    assert lib.avd_gate_fwd(None, 2 * E, d, d, d, 2 * E, 4, E, None) == -4
    assert lib.avd_gate_fwd(d, 2 * E - 1, d, d, d, 2 * E, 4, E, None) == -1
    assert lib.avd_gate_fwd(d, 2 * E, d, d, d, 2 * E, 0, E, None) == -1
    assert lib.avd_gate_bwd_ws(300, E) == 2 * 10 and lib.avd_gate_bwd_ws(0, E) == -1
    assert lib.avd_gate_bwd(d, 2 * E, d, 2 * E, d, d, d, 2 * E, d, None, d, 2, 4, E, None) == -4
    assert lib.avd_gate_bwd(d, 2 * E, d, 2 * E, d, d, d, 2 * E, d, d, d, 1, 4, E, None) == -4    # ws too small
    assert lib.avd_gate_bwd(d, 2 * E, d, 2 * E, d, d, d, E, d, d, d, 2, 4, E, None) == -1
    assert lib.avd_softmax_rows_fwd(None, 8, 4, 8, None) == -4
    assert lib.avd_softmax_rows_fwd(d, 7, 4, 8, None) == -1
    assert lib.avd_softmax_rows_bwd(d, 8, None, 8, 4, 8, None) == -4
    assert lib.avd_softmax_rows_bwd(d, 8, d, 8, 0, 8, None) == -1


def test_ops_wrappers_check_bounds_on_the_host():
    """ops.xattn_fwd rejects operands the kernel would read or write out of bounds, before any
    launch (CPU tensors: a launch would fail differently)."""
    from avdino import ops
    E, B, groups = 32, 5, 2
    rows = groups * B
    qkv, x = torch.zeros(rows * 3 * E), torch.zeros(rows * 2 * E)
    out = torch.zeros((rows - 1) * 2 * E + E - 1)         # one element short of the last owned row
    q, k, v = ((qkv, c * E, 3 * E, 0) for c in range(3))
    with pytest.raises(ValueError, match="out bounds"):
        ops.xattn_fwd(q, k, v, (x, 0, 2 * E, 0), (out, 0, 2 * E, 0), None, 1, groups, B, E, 0.1)
    with pytest.raises(ValueError, match="one of"):
        ops.xattn_fwd(q, k, v, (x, 0, 2 * E, 0), (x, 0, 2 * E, 0), None, 1, groups, B, 48, 0.1)
    with pytest.raises(ValueError, match="x bounds"):
        ops.xattn_fwd(q, k, v, (x, E, 2 * E, E), (x, 0, 2 * E, 0), None, 2, groups, B, E, 0.1)
