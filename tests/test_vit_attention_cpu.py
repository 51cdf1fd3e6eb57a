"""The ViT tower's attention choice ("exact" = avd_mhsa_*, "mfma" = avd_mhsa_mfma_*) through the
Python layers, without a device: defaults, refusals, the command line down to the model and its
checkpoint, the kernels' dispatch table and the ops wrappers' host-side checks."""
import os

import pytest
import torch

from avdino import ops
from avdino._lib import lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(REPO, "configs", "config_multimodal_dino.yaml")
DIMS = dict(hw=112, patch=8, embed_dim=512, depth=4, heads=4)
BF16, F32 = torch.bfloat16, torch.float32


def cli(*extra):
    from avdino import run_dino as R
    return R.parse_args(["--config", CFG, *extra])


def test_defaults_are_exact_at_every_layer():
    from avdino import models as M
    from avdino.engine import UniEncoder
    from avdino.vit import ATTENTION_KINDS, ViTTower
    assert ATTENTION_KINDS == ("exact", "mfma")
    for act in (F32, BF16):
        assert ViTTower("student.encoder.0", act_dtype=act, gemm_mode=0, **DIMS).attention == "exact"
        enc = UniEncoder("spectrogram_vit", "student", act, 0, out_dim=32)
        assert enc.vit_attention == "exact" and enc.tower.attention == "exact"
    assert UniEncoder("spectrogram_simple", "student", BF16, 0).vit_attention == "exact"
    assert M.SpectrogramEncoderViT().attention == "exact" and M.SpectrogramEncoderViT(64).output_dim == 64
    assert cli("--unimodal_model", "spectrogram_vit").vit_attention == "exact"
    assert cli("--model", "multi_central").vit_attention == "exact"


def test_mfma_reaches_the_towers():
    from avdino import models as M
    from avdino.engine import UniEncoder
    from avdino.vit import ViTTower
    assert ViTTower("p", act_dtype=BF16, gemm_mode=0, attention="mfma", **DIMS).attention == "mfma"
    assert UniEncoder("spectrogram_vit", "teacher", BF16, 0, out_dim=32, vit_attention="mfma").tower.attention == "mfma"
    assert M.SpectrogramEncoderViT(64, attention="mfma").attention == "mfma"


def test_unknown_kind_and_f32_with_mfma_raise():
    from avdino import models as M
    from avdino.engine import UniEncoder
    from avdino.vit import ViTTower
    with pytest.raises(ValueError, match="one of"):
        ViTTower("p", act_dtype=BF16, gemm_mode=0, attention="flash", **DIMS)
    with pytest.raises(ValueError, match="bf16"):
        ViTTower("p", act_dtype=F32, gemm_mode=0, attention="mfma", **DIMS)
    with pytest.raises(ValueError, match="one of"):
        UniEncoder("spectrogram_vit", "student", BF16, 0, out_dim=32, vit_attention="flash")
    with pytest.raises(ValueError, match="bf16"):
        UniEncoder("spectrogram_vit", "student", F32, 0, out_dim=32, vit_attention="mfma")
    with pytest.raises(ValueError, match="no ViT tower"):
        UniEncoder("spectrogram_simple", "student", BF16, 0, vit_attention="mfma")
    with pytest.raises(ValueError, match="one of"):
        M.SpectrogramEncoderViT(attention="flash")
    with pytest.raises(ValueError, match="bf16"):
        M.UniModalDINO(encoder_class=M.SpectrogramEncoderViT, encoder_kwargs={"attention": "mfma"}, output_dim=32,
                       projection_dim=16, device="cpu", precision="32")


def test_command_line_refusals():
    with pytest.raises(SystemExit):
        cli("--unimodal_model", "spectrogram_vit", "--vit-attention", "mfma", "--precision", "32")
    with pytest.raises(SystemExit):
        cli("--unimodal_model", "spectrogram_simple", "--vit-attention", "mfma")
    with pytest.raises(SystemExit):
        cli("--model", "multi_central", "--vit-attention", "mfma")
    with pytest.raises(SystemExit):
        cli("--unimodal_model", "spectrogram_vit", "--vit-attention", "flash")
    assert cli("--unimodal_model", "spectrogram_vit", "--vit-attention", "exact", "--precision", "32").precision == "32"


def test_command_line_to_model_and_checkpoint(tmp_path):
    from avdino import models as M
    from avdino import run_dino as R
    from avdino.downstream import _probe_kwargs
    from avdino.trainer import load_checkpoint, save_checkpoint
    cfg = R.load_config(CFG)
    a = cli("--unimodal_model", "spectrogram_vit", "--vit-attention", "mfma")
    assert a.vit_attention == "mfma" and a.precision == "bf16"
    m = R.build_model(a, cfg, device="cpu")
    assert type(m.model.student_spec) is M.SpectrogramEncoderViT and m.model.student_spec.attention == "mfma"
    assert m.model.vit_attention == "mfma" and m.model.student.vit_attention == "mfma"
    assert dict(m.hparams)["encoder_kwargs"] == {"attention": "mfma"}
    assert _probe_kwargs(m, True) == {"vit_attention": "mfma"} == _probe_kwargs(m.model, True)
    path = str(tmp_path / "mfma.ckpt")
    save_checkpoint(m, path, epoch=1, global_step=2)
    ck = load_checkpoint(path)
    assert ck["hyper_parameters"]["encoder_kwargs"] == {"attention": "mfma"}
    m2 = M.UniModalDINOLightning.load_from_checkpoint(path, device="cpu")
    assert m2.model.vit_attention == "mfma" and m2.model.student_spec.attention == "mfma"
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    # the default changes nothing that is saved, and hyper-parameters without the key are "exact"
    d = R.build_model(cli("--unimodal_model", "spectrogram_vit"), cfg, device="cpu")
    assert dict(d.hparams)["encoder_kwargs"] is None and d.model.vit_attention == "exact"
    assert _probe_kwargs(d, True) == {}
    old = str(tmp_path / "old.ckpt")
    save_checkpoint(d, old, epoch=1, global_step=2)
    ck = load_checkpoint(old)
    hp = dict(ck["hyper_parameters"])
    hp.pop("encoder_kwargs")                  # a checkpoint that never heard of encoder_kwargs
    ck["hyper_parameters"] = hp
    torch.save(ck, old)
    m3 = M.UniModalDINOLightning.load_from_checkpoint(old, device="cpu")
    assert m3.model.vit_attention == "exact" and m3.model.student_spec.attention == "exact"


def test_dispatch_table_is_that_of_the_exact_kernels():
    ts = (1, 255, 256, 257)
    ok = {(dh, T) for dh in range(1, 161) for T in ts if lib.avd_mhsa_mfma_bwd_ws(2, 3, T, dh) > 0}
    assert ok == {(dh, T) for dh in ops.MHSA_HEAD_DIMS for T in ts if T <= ops.MHSA_TMAX}
    assert all(lib.avd_mhsa_mfma_bwd_ws(2, 3, T, dh) == -1 for dh in range(1, 161) for T in ts if (dh, T) not in ok)
    assert lib.avd_mhsa_mfma_bwd_ws(2, 3, 0, 32) == -1 and lib.avd_mhsa_mfma_bwd_ws(0, 3, 5, 32) == -1
    assert lib.avd_mhsa_mfma_bwd_ws(2, 3, 197, 128) == ops.mhsa_mfma_bwd_ws(2, 3, 197, 128) == 2 * 3 * 197
    from tests import test_gpu_mhsa_mfma as TM
    assert ops.MHSA_TMAX in TM.MFMA_TS and ops.MHSA_TMAX - 1 in TM.MFMA_TS and max(TM.MFMA_TS) == ops.MHSA_TMAX
    assert all(dh in ops.MHSA_HEAD_DIMS and T <= ops.MHSA_TMAX for _n, _h, T, dh, _p in TM.MFMA_DROPOUT_CASES)


def test_ops_wrappers_check_on_the_host():
    """CPU tensors: anything that reached the library would fail differently."""
    N, heads, T, dh = 2, 2, 5, 32
    E, R = heads * dh, N * T
    qkv, ctx, lse = torch.zeros(R * 3 * E), torch.zeros(R * E), torch.zeros(N * heads * T)
    q, k, v = (qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E)
    ws = torch.zeros(N * heads * T)
    with pytest.raises(ValueError, match="one of"):
        ops.mhsa_mfma_fwd(q, k, v, (ctx, 0, E), lse, N, 1, T, 48, 0.1)
    with pytest.raises(ValueError, match="T <= 256"):
        ops.mhsa_mfma_fwd(q, k, v, (ctx, 0, E), lse, N, heads, 257, dh, 0.1)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.mhsa_mfma_fwd(q, (qkv, E, 3 * E + 2), v, (ctx, 0, E), lse, N, heads, T, dh, 0.1)
    with pytest.raises(ValueError, match="ctx bounds"):
        ops.mhsa_mfma_fwd(q, k, v, (ctx[:-1], 0, E), lse, N, heads, T, dh, 0.1)
    with pytest.raises(ValueError, match="dropout"):
        ops.mhsa_mfma_fwd(q, k, v, (ctx, 0, E), lse, N, heads, T, dh, 0.1, drop_p=1.0)
    with pytest.raises(ValueError, match="one of"):
        ops.mhsa_mfma_bwd_ws(N, 1, T, 48)
    with pytest.raises(ValueError, match="T <= 256"):
        ops.mhsa_mfma_bwd_ws(N, heads, 257, dh)
    with pytest.raises(ValueError, match="one of"):
        ops.mhsa_mfma_bwd((ctx, 0, E), q, k, v, lse, q, k, v, ws, N, 1, T, 48, 0.1)
    with pytest.raises(ValueError, match="T <= 256"):
        ops.mhsa_mfma_bwd((ctx, 0, E), q, k, v, lse, q, k, v, ws, N, heads, 257, dh, 0.1)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.mhsa_mfma_bwd((ctx, 0, E), q, k, v, lse, q, (qkv, E, 3 * E + 2), v, ws, N, heads, T, dh, 0.1)
    with pytest.raises(ValueError, match="workspace"):
        ops.mhsa_mfma_bwd((ctx, 0, E), q, k, v, lse, q, k, v, ws[:-1], N, heads, T, dh, 0.1)
