"""The audio CNN+LSTM encoder (spectrogram_lstm) without a GPU: the float64 restatement
tests/lstm_ref.py is pinned to the reference's float64 fixtures, and the spec, initialisation,
checkpoint, command-line and argument-validation surface of the new encoder."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle.params import make_multimodal_batch
from tests import golden_util as gu
from tests import lstm_ref as LR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(REPO, "configs", "config_multimodal_dino.yaml")
D, P, B, G, L = (LR.DIMS[k] for k in "DPBGL")


def _check(fx, key, value, rel=1e-8):
    ok, msg = gu.compare(fx, key, value, rel=rel)
    assert ok, msg


@pytest.fixture(scope="module")
def ref_step():
    spec = LR.lstm_spec(D, P)
    state = LR.lstm_state(spec, LR.PSEED)
    batch = make_multimodal_batch(B, G, L, LR.BSEED, with_originals=False)
    return spec, state, LR.unimodal_step(state, batch, LR.HP, spec)


def test_lstm_ref_reproduces_the_float64_fixture(ref_step):
    spec, state, r = ref_step
    fx = gu.load(LR.NAME + "_f64")
    assert abs(r["loss"] - float(fx["loss"])) < 1e-8
    _check(fx, "s_out", r["s_out"])
    _check(fx, "t_out", r["t_out"])
    _check(fx, "emb", r["emb"])
    assert sorted(r["grads"]) == sorted(str(k) for k in fx["live_keys"])
    zero = gu.zero_grad_keys(fx)
    for k, g in r["grads"].items():
        if "grad/" + k in zero:
            assert np.linalg.norm(g) < 1e-9, k
            assert "feature_proj" not in k and ".lstm." not in k
        else:
            _check(fx, "grad/" + k, g)
    np.testing.assert_allclose(r["center_after"], fx["center_after"], atol=1e-10, rtol=0)
    new = r["state"]
    for k in spec:
        if k.endswith("running_mean") or k.endswith("running_var"):
            _check(fx, "rs/" + k, new[k])
        elif k.startswith("teacher") and not k.endswith("num_batches_tracked"):
            _check(fx, "ema/" + k, new[k])
    post = LR.adam_update(new, r["grads"], {}, 1, LR.HP)
    for k in r["grads"]:
        _check(fx, "post/" + k, post[k])


def test_lstm_ref_loss_curve_and_eval_features():
    spec = LR.lstm_spec(D, P)
    st = LR.lstm_state(spec, LR.PSEED)
    opt, curve = {}, []
    for step in range(LR.STEPS):
        b = make_multimodal_batch(B, G, L, LR.BSEED + step, with_originals=False)
        r = LR.unimodal_step(st, b, LR.HP, spec)
        curve.append(r["loss"])
        st = LR.adam_update(r["state"], r["grads"], opt, step + 1, LR.HP)
    np.testing.assert_allclose(curve, gu.load(LR.NAME + "_f64")["curve"], atol=1e-8, rtol=0)
    fx = gu.load(LR.EVAL_NAME + "_f64")
    assert tuple(fx["meta_batches"]) == LR.EVAL_BATCHES
    state = LR.lstm_state(spec, LR.PSEED, stats=True)
    for i, n in enumerate(LR.EVAL_BATCHES):
        x = make_multimodal_batch(n, 1, 1, LR.EVAL_SEED + i)["audio"]
        f = LR.eval_features(state, x)
        assert f.shape == (n, D)
        assert gu.rel_err(f, fx[f"feat{i}"]) < 1e-8


def test_state_dict_keys_order_and_shapes():
    from avdino.models import SpectrogramEncoderLSTM, UniModalDINO
    ref = json.load(open(os.path.join(gu.GOLDEN, "lstm_state_keys.json")))[f"spectrogram_lstm/D{D}_P{P}"]
    spec = LR.lstm_spec(D, P)
    assert [[k, list(shp)] for k, (shp, _kind) in spec.items()] == ref
    m = UniModalDINO(encoder_class=SpectrogramEncoderLSTM, output_dim=D, projection_dim=P, device="cpu")
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref
    lstm = [k for k, _ in ref if k.startswith("student.encoder.lstm.")]
    assert lstm == ["student.encoder.lstm." + n for n in LR.LSTM_NAMES]


def test_lstm_initialisation_is_uniform_in_one_over_sqrt_hidden():
    from avdino.params import ParamStore
    Dd = 64
    H = Dd // 2
    store = ParamStore(LR.lstm_spec(Dd, P), "cpu", seed=3)
    bound = 1.0 / math.sqrt(H)
    for n in LR.LSTM_NAMES:
        w = store["student.encoder.lstm." + n]
        assert w.shape[0] == 4 * H
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound, n
        assert float(w.std()) > 0.4 * bound, n                 # not constant: U(-b, b) has b / sqrt 3
        assert torch.equal(w, store["teacher.encoder.lstm." + n])
    fp = store["student.encoder.feature_proj.0.weight"]
    assert float(fp.abs().max()) <= 1.0 / math.sqrt(128)


def test_checkpoint_round_trip(tmp_path):
    from avdino import models as M
    from avdino.trainer import load_checkpoint, save_checkpoint
    enc = M.SpectrogramEncoderLSTM
    m = M.UniModalDINOLightning(encoder_class=enc, output_dim=D, projection_dim=P, device="cpu")
    spec = LR.lstm_spec(D, P)
    m.load_state_dict({"model." + k: torch.from_numpy(np.array(v))
                       for k, v in LR.lstm_state(spec, 5).items()})
    path = str(tmp_path / "x.ckpt")
    save_checkpoint(m, path, epoch=3, global_step=12)
    assert load_checkpoint(path)["hyper_parameters"]["encoder_class"] == enc.__name__
    m2 = M.UniModalDINOLightning.load_from_checkpoint(path, device="cpu")
    assert type(m2.model.student_spec) is enc
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    bad = dict(m.state_dict())
    bad.pop("model.teacher.encoder.lstm.weight_hh_l0_reverse")
    with pytest.raises(RuntimeError, match="Missing"):
        m2.load_state_dict(bad)


@pytest.mark.parametrize("dim", [31, 16, 40, 288, 0])
def test_unsupported_output_dim_is_refused_with_the_list(dim):
    from avdino import models as M
    with pytest.raises(ValueError, match=r"\(32, 64, 96, 128, 160, 192, 224, 256\)"):
        M.UniModalDINO(encoder_class=M.SpectrogramEncoderLSTM, output_dim=dim, projection_dim=P,
                       device="cpu")
    from avdino.spec import unimodal_dino_sd
    with pytest.raises(ValueError, match=r"\(32, 64, 96, 128, 160, 192, 224, 256\)"):
        unimodal_dino_sd("spectrogram_lstm", dim, P)


def test_model_map_cli_and_submit_models(capsys):
    from avdino import models as M
    from avdino import run_dino as R
    from avdino import submit_models as SM
    assert M.UNIMODAL_MODEL_MAP["spectrogram_lstm"] is M.SpectrogramEncoderLSTM
    assert M.SpectrogramEncoderLSTM.modality == "audio" and M.SpectrogramEncoderLSTM(64).output_dim == 64
    cfg = R.load_config(CFG)
    a = R.parse_args(["--unimodal_model", "spectrogram_lstm", "--config", CFG, "--precision", "32"])
    m = R.build_model(a, cfg, device="cpu")
    assert type(m) is M.UniModalDINOLightning
    assert type(m.model.student_spec) is M.SpectrogramEncoderLSTM
    cmds = SM.main(["--models", "spectrogram_lstm", "--config", CFG, "--dry-run"])
    assert cmds[0][1:] == ["-m", "avdino.run_dino", "--unimodal_model", "spectrogram_lstm", "--config", CFG,
                           "--metric", "mlp_acc"]
    assert capsys.readouterr().out.count("Submitting:") == 1
    for name in ("multi_lstm", "spectrogram_vit", "spectrogram_resnet", "multi_mobile_vit"):
        with pytest.raises(SystemExit):
            SM.main(["--models", name, "--config", CFG, "--dry-run"])


def test_model_stats_parameters_and_macs():
    """The parameter count is the reference's (the sum over lstm_state_keys.json's parameter
    tensors); the LSTM's multiply-adds follow the formula in model_stats' docstring."""
    from avdino import models as M
    from avdino import run_dino as R
    ref = json.load(open(os.path.join(gu.GOLDEN, "lstm_state_keys.json")))[f"spectrogram_lstm/D{D}_P{P}"]
    nparam = sum(int(np.prod(shp)) for k, shp in ref
                 if not k.endswith(("running_mean", "running_var", "num_batches_tracked")) and k != "center")
    m = M.UniModalDINOLightning(encoder_class=M.SpectrogramEncoderLSTM, output_dim=D, projection_dim=P,
                                device="cpu")
    gflops, params = R.model_stats(m, 2, 4)
    assert params == nparam
    H, T = D // 2, 196
    conv = 112 * 112 * 32 * 9 + 56 * 56 * 64 * 32 * 9 + 28 * 28 * 128 * 64 * 9
    enc = conv + T * 128 * 64 + T * 2 * 4 * H * (64 + H)
    head = D * 512 + 512 * P
    assert gflops == pytest.approx((6 + 2) * (enc + head) / 1e9, rel=1e-12)


def test_lstm_argument_validation_without_launch():
    from avdino._lib import lib
    d = ctypes.c_void_p(4096)
    a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
    assert lib.avd_lstm_ws(3, 196, 16, ctypes.byref(a), ctypes.byref(b)) == 0
    assert a.value == 3 * 196 * 2 * 6 * 16 and b.value == 3 * 196 * 2 * 4 * 16
    assert lib.avd_lstm_ws(3, 196, 16, None, ctypes.byref(b)) == -4
    for H in (0, 8, 24, 144, 256):
        assert lib.avd_lstm_ws(3, 196, H, ctypes.byref(a), ctypes.byref(b)) == -1

    def fwd(gx=d, out=d, save=d, flag=1, dt=0, N=3, T=5, H=16):
        return lib.avd_lstm_fwd(gx, d, d, out, save, flag, dt, N, T, H, None)

    assert fwd(gx=None) == -4 and fwd(out=None) == -4 and fwd(save=None) == -4
    assert fwd(dt=2) == -2 and fwd(dt=-1) == -2
    assert fwd(H=24) == -1 and fwd(H=144) == -1 and fwd(N=0) == -1 and fwd(T=0) == -1
    assert fwd(save=None, flag=0, H=24) == -1          # no save buffer needed without save

    def bwd(dout=d, save=d, dg=d, dt=1, N=3, T=5, H=32):
        return lib.avd_lstm_bwd(dout, d, d, save, dg, dt, N, T, H, None)

    assert bwd(dout=None) == -4 and bwd(save=None) == -4 and bwd(dg=None) == -4
    assert bwd(dt=3) == -2 and bwd(H=8) == -1 and bwd(N=0) == -1 and bwd(T=-1) == -1
    assert lib.avd_cast(None, 1, d, 0, 4, None) == -4 and lib.avd_cast(d, 1, d, 0, 0, None) == -1
    assert lib.avd_cast(d, 0, d, 0, 4, None) == -2


def test_ops_lstm_wrappers_check_sizes_on_the_host():
    """ops.lstm_* reject operands the kernel would read or write out of bounds before any launch
    (CPU tensors: a launch would fail differently)."""
    from avdino import ops
    N, T, H = 3, 4, 16
    ns, ng = ops.lstm_ws(N, T, H)
    assert (ns, ng) == (N * T * 2 * 6 * H, N * T * 2 * 4 * H)
    assert ops.lstm_hprev_offset(N, T, H) == N * T * 2 * 5 * H
    gx, w, out, save = torch.zeros(ng), torch.zeros(4 * H * H), torch.zeros(N * 2 * H), torch.zeros(ns)
    with pytest.raises(ValueError, match="one of"):
        ops.lstm_fwd(gx, w, w, out, save, N, T, 24, False)
    with pytest.raises(ValueError, match="gx"):
        ops.lstm_fwd(gx[:-1], w, w, out, save, N, T, H, False)
    with pytest.raises(ValueError, match="out"):
        ops.lstm_fwd(gx, w, w, out[:-1], save, N, T, H, False)
    with pytest.raises(ValueError, match="saved state"):
        ops.lstm_fwd(gx, w, w, out, save[:-1], N, T, H, True)
    with pytest.raises(ValueError, match="weight_hh"):
        ops.lstm_fwd(gx, w[:-1], w, out, None, N, T, H, True)
    with pytest.raises(ValueError, match="gx"):
        ops.lstm_fwd(gx.double(), w, w, out, None, N, T, H, False)
    with pytest.raises(ValueError, match="dg"):
        ops.lstm_bwd(out, w, w, save, gx[:-1], N, T, H, False)
    with pytest.raises(ValueError, match="saved state"):
        ops.lstm_bwd(out, w, w, None, gx, N, T, H, False)
    with pytest.raises(ValueError, match="N, T"):
        ops.lstm_ws(0, T, H)
    with pytest.raises(ValueError, match="cast"):
        ops.cast(torch.zeros(4), torch.zeros(4), 4)
    with pytest.raises(ValueError, match="cast bounds"):
        ops.cast(torch.zeros(4), torch.zeros(3, dtype=torch.bfloat16), 4)
