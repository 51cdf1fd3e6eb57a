"""spectrogram_lstm training-step parity: the HIP engine (UniModalEngine over the audio CNN+LSTM
encoder, fp32 parity mode) vs tests/lstm_ref.py (float64 torch on the CPU, pinned to the
reference's float64 fixture by tests/test_lstm_cpu.py), from identical parameters and inputs at
the fixture's dimensions (D = 32, P = 16, B = 3, 2 global + 2 local views).

Bands, those of test_gpu_uni.py: loss 3e-5 abs; outputs and embeddings max(1e-5, 3x the
reference's own fp32-vs-float64 error, from the two fixtures); gradients max(1e-3, 3x that error
per tensor), median 1e-4; EMA'd teacher 1e-6; running statistics 1e-5; post-Adam parameters 1e-6.
The absolute near-zero check (1e-4) is taken only by the three conv biases that feed a
BatchNorm2d; every feature_proj and lstm tensor takes the relative check.  One more gradient is
mathematically zero and so has no relative error: the projection head's mlp.0 bias, which feeds
its BatchNorm1d (4e-13 in float64).  What is left there is the rounding residue of 512 cancelling
column sums, 1.2e-4 in the reference's own fp32 run at these dimensions, so its absolute band is
max(1e-4, 3x that residue), the 3x-the-reference's-own-error rule of the other tensors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle.params import make_multimodal_batch  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import lstm_ref as LR  # noqa: E402

D, P, B, G, L = (LR.DIMS[k] for k in "DPBGL")
HP = LR.HP
# gradients that are mathematically zero: a bias whose output reaches the loss only through a
# train-mode BatchNorm
ZERO_GRAD = {"student.encoder.cnn.0.bias", "student.encoder.cnn.4.bias", "student.encoder.cnn.8.bias"}
HEAD_BIAS = "student_projection.mlp.0.bias"


def rel(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def fp32_err(key):
    """rel-L2 error of the reference's fp32 run vs its float64 run on a fixture tensor."""
    f32, f64 = gu.load(LR.NAME), gu.load(LR.NAME + "_f64")
    if key in f64:
        return gu.rel_err(f32[key], f64[key])
    return gu.rel_err(f32[key + "@val"], f64[key + "@val"])


def build(Dd=D, Pp=P, pseed=LR.PSEED, act=torch.float32, stats=False):
    from avdino.engine import Hyper, UniModalEngine
    from avdino.params import ParamStore
    spec = LR.lstm_spec(Dd, Pp)
    store = ParamStore(spec, "cuda")
    state = LR.lstm_state(spec, pseed, stats=stats)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    hp = Hyper(lr=HP["lr"], weight_decay=HP["wd"], momentum=HP["momentum"],
               center_momentum=HP["center_momentum"], student_temperature=HP["tau_s"],
               teacher_temperature=HP["tau_t"], dropout=0.0, fusion_dropout=0.0)
    return spec, store, UniModalEngine(store, LR.KIND, Dd, Pp, hp, act_dtype=act), state


def dev_batch(b):
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}


@pytest.fixture(scope="module")
def ref_step():
    """The float64 step on the fixture case: computed once, shared, never modified."""
    spec = LR.lstm_spec(D, P)
    state = LR.lstm_state(spec, LR.PSEED)
    batch = make_multimodal_batch(B, G, L, LR.BSEED, with_originals=False)
    return batch, LR.unimodal_step(state, batch, HP, spec)


def test_fp32_step_matches_the_float64_restatement(ref_step):
    from avdino.engine import adam_step, ema_step
    batch, ref = ref_step
    assert abs(ref["loss"] - float(gu.load(LR.NAME + "_f64")["loss"])) < 1e-8
    spec, store, eng, _state = build()
    loss = eng.forward(dev_batch(batch))
    s_out, t_out, emb = eng.outputs()
    assert abs(loss.item() - ref["loss"]) < 3e-5, (loss.item(), ref["loss"])
    obound = max(1e-5, 3 * fp32_err("s_out"), 3 * fp32_err("t_out"), 3 * fp32_err("emb"))
    errs = {k: rel(host(v), ref[k]) for k, v in (("s_out", s_out), ("t_out", t_out), ("emb", emb))}
    print("outputs", errs, "bound", obound)
    assert all(e < obound for e in errs.values()), (errs, obound)
    eng.update_center()
    assert rel(host(store["center"]), ref["center_after"]) < 1e-5
    ema_step(store, HP["momentum"])
    eng.backward()
    assert sorted(store.live_keys) == sorted(ref["grads"].keys())
    errs = {}
    for k in store.live_keys:
        g, r = host(store.grad_of(k)), ref["grads"][k]
        if k in ZERO_GRAD or k == HEAD_BIAS:
            floor = 1e-4
            if k == HEAD_BIAS:
                floor = max(floor, 3 * float(np.linalg.norm(gu.load(LR.NAME)["grad/" + k])))
            assert np.linalg.norm(r) < 1e-9 and np.linalg.norm(g - r) <= floor, (k, np.linalg.norm(g - r))
            continue
        assert np.linalg.norm(r) >= 1e-4, k
        errs[k] = rel(g, r)
        bound = max(1e-3, 3 * fp32_err("grad/" + k))
        assert errs[k] < bound, (k, errs[k], bound)
    assert all(k in errs for k in store.live_keys if "feature_proj" in k or ".lstm." in k)
    print("worst grad errors:", sorted(errs.items(), key=lambda kv: -kv[1])[:6])
    assert np.median(list(errs.values())) < 1e-4
    new = ref["state"]
    for k in store.t_offs:
        assert rel(host(store[k]), new[k]) < 1e-6, k
    for k in store.buffers:
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert rel(host(store.buffers[k]), new[k]) < 1e-5, k
        elif k.endswith("num_batches_tracked"):
            assert int(store.buffers[k].item()) == int(new[k]), k
    ours = {k: host(store.grad_of(k)) for k in store.live_keys}
    pre = {k: host(store[k]) for k in store.live_keys}
    adam_step(store, eng.hp)
    post = LR.adam_update(pre, ours, {}, 1, HP)
    for k in store.live_keys:
        assert rel(host(store[k]), post[k]) < 1e-6, k


def test_three_step_loss_curve():
    """Every step's loss equals the restatement's on the engine's own state, and the free-running
    curve stays within the fp32 band of the fixture's."""
    spec, store, eng, state = build()
    golden = gu.load(LR.NAME + "_f64")["curve"]
    curve, from_ours = [], []
    for step in range(LR.STEPS):
        b = make_multimodal_batch(B, G, L, LR.BSEED + step, with_originals=False)
        ours = {k: store[k].detach().cpu().numpy() for k in spec}
        from_ours.append(LR.unimodal_step(ours, b, HP, spec)["loss"])
        curve.append(eng.step(dev_batch(b)).item())
    print("curve", curve, "restated on our state", from_ours, "reference f64", golden)
    np.testing.assert_allclose(curve, from_ours, atol=3e-5, rtol=0)
    np.testing.assert_allclose(curve, golden, atol=1e-3, rtol=0)


def test_bf16_step_close_to_the_restatement():
    """The bands test_gpu_uni.py's bf16 step uses for spectrogram_simple."""
    Dd, Pp, Bb = 64, 32, 4
    spec, store, eng, state = build(Dd, Pp, 321, act=torch.bfloat16)
    batch = make_multimodal_batch(Bb, 2, 2, 3210, with_originals=False)
    ref = LR.unimodal_step(state, batch, HP, spec)
    loss = eng.forward(dev_batch(batch))
    assert abs(loss.item() - ref["loss"]) < 2e-2 * abs(ref["loss"])
    eng.update_center()
    eng.backward()
    errs = sorted(((rel(host(store.grad_of(k)), ref["grads"][k]), k) for k in store.live_keys
                   if np.linalg.norm(ref["grads"][k]) > 1e-4), reverse=True)
    med = np.median([e for e, _ in errs])
    print("bf16 loss", loss.item(), ref["loss"], "median", med, "worst", errs[:6])
    assert any(".lstm." in k for _, k in errs) and any("feature_proj" in k for _, k in errs)
    assert med < 0.2 and errs[0][0] < 0.6, (med, errs[:6])


@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16])
def test_graph_step_is_bitwise_the_eager_step(act):
    """Five steps: the graphed engine runs its two warm-up steps eagerly, captures at the third
    and replays; all five, and the state after them, equal the eager engine's bit for bit."""
    batches = [make_multimodal_batch(B, G, L, 90 + s, with_originals=False) for s in range(5)]
    runs = []
    for graph in (False, True):
        _spec, store, eng, _ = build(act=act)
        eng.use_graph = graph
        losses = [eng.step(dev_batch(b)).clone() for b in batches]
        torch.cuda.synchronize()
        assert eng.graph.captures == (1 if graph else 0)
        runs.append((torch.stack(losses).cpu(), store.student.clone().cpu(), store.teacher.clone().cpu(),
                     store.buf_arena.clone().cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]).all()


def test_eval_features_match_the_fixture_including_the_ragged_batch():
    spec, store, eng, state = build(stats=True)
    fx = gu.load(LR.EVAL_NAME + "_f64")
    bound = max(1e-5, 3 * gu.rel_err(gu.load(LR.EVAL_NAME)["feat0"], fx["feat0"]))
    for i, n in enumerate(LR.EVAL_BATCHES):
        x = make_multimodal_batch(n, 1, 1, LR.EVAL_SEED + i)["audio"]
        xs = torch.from_numpy(np.ascontiguousarray(x.reshape(n, 112, 112, 1))).cuda()
        f = eng.enc.forward_eval(eng.ws, store, "ev", xs.reshape(-1), n)
        assert f.shape == (n, D)
        assert rel(host(f), fx[f"feat{i}"]) < bound, (i, rel(host(f), fx[f"feat{i}"]), bound)


def test_lightning_step_probe_and_knn_run():
    """One UniModalDINOLightning.training_step, the epoch-end probe and the kNN classifier over
    the new encoder: shapes and finite values only."""
    from avdino import downstream as DS
    from avdino.models import UNIMODAL_MODEL_MAP, UniModalDINOLightning
    m = UniModalDINOLightning(encoder_class=UNIMODAL_MODEL_MAP["spectrogram_lstm"], output_dim=D,
                              projection_dim=P, dropout=0.0, precision="32", device="cuda")
    b = make_multimodal_batch(4, 2, 2, 77, with_originals=False)
    views = tuple(torch.from_numpy(b[k]) for k in ("g_img", "g_aud", "l_img", "l_aud"))
    opt = m.configure_optimizers()["optimizer"]
    pre = m.model.store.student.clone()
    loss = m.training_step(views, 0)
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert np.isfinite(loss.item()) and not torch.equal(pre, m.model.store.student)

    def loader(n, seed):
        out = []
        for j in range(n):
            bb = make_multimodal_batch(6, 1, 0, seed + j)
            out.append(tuple(torch.from_numpy(bb[k]).cuda() for k in ("image", "audio", "label")))
        return out

    train, valid = loader(2, 500), loader(1, 600)
    m.on_train_epoch_end(train, valid)
    assert np.isfinite(m.logged["val_loss"]) and 0.0 <= m.logged["mlp_acc"] <= 100.0    # per cent
    feats, labels = DS.feature_extraction_loop("cuda", DS.FeatureExtractor(m.model), train)
    assert feats.shape == (12, D) and labels.shape == (12,) and bool(torch.isfinite(feats).all())
    knn, acc = DS.train_knn_classifier(m.model, train, valid, n_neighbors=3)
    assert knn.predict(feats).shape == (12,) and 0.0 <= float(acc) <= 100.0
