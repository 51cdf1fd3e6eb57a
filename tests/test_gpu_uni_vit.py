"""spectrogram_vit training-step parity: the HIP engine (UniModalEngine over the audio ViT encoder,
fp32 parity mode) vs tests/vit_ref.py (float64 torch on the CPU, pinned to the reference's float64
fixture by tests/test_vit_cpu.py), from identical parameters and inputs at the fixture's
dimensions (D = 32, P = 16, B = 3, 2 global + 2 local views: 12 student sequences of 197 tokens).
The file mirrors tests/test_gpu_uni_lstm.py test for test, with its bands.

Bands: loss 3e-5 abs; outputs and embeddings max(1e-5, 3x the reference's own fp32-vs-float64
error, from the two fixtures); gradients max(1e-3, 3x that error per tensor), median 1e-4, the
attention in-projection's weight and bias compared per q / k / v third; EMA'd teacher 1e-6; running
statistics 1e-5; post-Adam parameters 1e-6.

Gradients that are mathematically zero have no relative error and take an absolute check instead
(tests/vit_ref.py ZERO_K_BIAS, ZERO_BN_BIAS):
  - the k third of the four in_proj_bias tensors (a constant added to every key's score leaves the
    softmax unchanged): floor 1e-4;
  - the projection head's mlp.0 bias, which feeds its BatchNorm1d: floor max(1e-4, 3x the residue
    in the reference's own fp32 fixture), as tests/test_gpu_uni_lstm.py;
  - and two more that this encoder adds in front of that BatchNorm1d through linear maps only --
    the final LayerNorm's bias and the Linear(512, D) bias behind it: each shifts every row of the
    head's input by one vector, which the batch statistics remove (5e-15 and 7e-15 in float64).
    They take the head bias's floor rule, each with its own fixture residue.
Every other tensor of the tower must take the relative check; the test asserts that.

With vit_dropout = 0.1 no reference exists (the masks are this project's counter hash): the tests
there are determinism, seed sensitivity, fresh masks per graph replay and finiteness.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle.params import make_multimodal_batch  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import vit_ref as VR  # noqa: E402

D, P, B, G, L = (VR.DIMS[k] for k in "DPBGL")
HP = VR.HP


def rel(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def fixtures():
    """(fp32, float64) step fixtures, read once."""
    return gu.load(VR.NAME), gu.load(VR.NAME + "_f64")


def fp32_err(key):
    """rel-L2 error of the reference's fp32 run vs its float64 run on a fixture tensor."""
    f32, f64 = fixtures()
    if key in f64:
        return gu.rel_err(f32[key], f64[key])
    return gu.rel_err(f32[key + "@val"], f64[key + "@val"])


def fp32_residue(key):
    """Norm of a mathematically zero gradient in the reference's own fp32 run."""
    f32 = fixtures()[0]
    return float(np.linalg.norm(f32[key])) if key in f32 else float(f32[key + "@norm"])


def build(Dd=D, Pp=P, pseed=VR.PSEED, act=torch.float32, stats=False, vit_dropout=0.0, seed=0):
    from avdino.engine import Hyper, UniModalEngine
    from avdino.params import ParamStore
    spec = VR.vit_spec(Dd, Pp)
    store = ParamStore(spec, "cuda")
    state = VR.vit_state(spec, pseed, stats=stats)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    hp = Hyper(lr=HP["lr"], weight_decay=HP["wd"], momentum=HP["momentum"],
               center_momentum=HP["center_momentum"], student_temperature=HP["tau_s"],
               teacher_temperature=HP["tau_t"], dropout=0.0, fusion_dropout=0.0, vit_dropout=vit_dropout)
    return spec, store, UniModalEngine(store, VR.KIND, Dd, Pp, hp, act_dtype=act, seed=seed), state


def dev_batch(b):
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}


@pytest.fixture(scope="module")
def ref_step():
    """The float64 step on the fixture case: computed once, shared, never modified."""
    spec = VR.vit_spec(D, P)
    state = VR.vit_state(spec, VR.PSEED)
    batch = make_multimodal_batch(B, G, L, VR.BSEED, with_originals=False)
    return batch, VR.unimodal_step(state, batch, HP, spec)


def test_fp32_step_matches_the_float64_restatement(ref_step):
    from avdino.engine import adam_step, ema_step
    batch, ref = ref_step
    assert abs(ref["loss"] - float(gu.load(VR.NAME + "_f64")["loss"])) < 1e-8
    spec, store, eng, _state = build()
    loss = eng.forward(dev_batch(batch))
    s_out, t_out, emb = eng.outputs()
    print("loss", loss.item(), ref["loss"])
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
    errs, absolute = {}, set()
    for k in store.live_keys:
        for sfx, g in VR.grad_slices(k, host(store.grad_of(k))):
            r = dict(VR.grad_slices(k, ref["grads"][k]))[sfx]
            if VR.is_zero_grad(k, sfx):
                floor = 1e-4 if sfx == "#k" else max(1e-4, 3 * fp32_residue("grad/" + k))
                print(f"zero gradient {k}{sfx}: |ours| {np.linalg.norm(g):.2e} (floor {floor:.2e})")
                assert np.linalg.norm(r) < 1e-9 and np.linalg.norm(g - r) <= floor, (k, sfx, np.linalg.norm(g - r))
                absolute.add(k + sfx)
                continue
            assert np.linalg.norm(r) >= 1e-4, (k, sfx)
            errs[k + sfx] = rel(g, r)
            bound = max(1e-3, 3 * fp32_err("grad/" + k + sfx))
            assert errs[k + sfx] < bound, (k, sfx, errs[k + sfx], bound)
    # the absolute check is taken by the four k-bias thirds and the three biases in front of the
    # head's BatchNorm1d, and by nothing else: every other tensor of the tower is in errs
    assert absolute == {k + "#k" for k in VR.ZERO_K_BIAS} | set(VR.ZERO_BN_BIAS)
    tower = [k + sfx for k in store.live_keys if ".encoder." in k
             for sfx, _ in VR.grad_slices(k, ref["grads"][k])]
    assert len(tower) == 56 + 2 * 8 and all(k in errs or k in absolute for k in tower)
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
    post = VR.adam_update(pre, ours, {}, 1, HP)
    for k in store.live_keys:
        assert rel(host(store[k]), post[k]) < 1e-6, k


def test_three_step_loss_curve():
    """Every step's loss equals the restatement's on the engine's own state, and the free-running
    curve stays within the fp32 band of the fixture's."""
    spec, store, eng, state = build()
    golden = gu.load(VR.NAME + "_f64")["curve"]
    curve, from_ours = [], []
    for step in range(VR.STEPS):
        b = make_multimodal_batch(B, G, L, VR.BSEED + step, with_originals=False)
        ours = {k: store[k].detach().cpu().numpy() for k in spec}
        from_ours.append(VR.unimodal_step(ours, b, HP, spec)["loss"])
        curve.append(eng.step(dev_batch(b)).item())
    print("curve", curve, "restated on our state", from_ours, "reference f64", golden)
    np.testing.assert_allclose(curve, from_ours, atol=3e-5, rtol=0)
    np.testing.assert_allclose(curve, golden, atol=1e-3, rtol=0)


def test_bf16_step_close_to_the_restatement():
    """The bands test_gpu_uni.py's bf16 step uses for spectrogram_simple."""
    Dd, Pp, Bb = 64, 32, 4
    spec, store, eng, state = build(Dd, Pp, 321, act=torch.bfloat16)
    batch = make_multimodal_batch(Bb, 2, 2, 3210, with_originals=False)
    ref = VR.unimodal_step(state, batch, HP, spec)
    loss = eng.forward(dev_batch(batch))
    assert abs(loss.item() - ref["loss"]) < 2e-2 * abs(ref["loss"])
    eng.update_center()
    eng.backward()
    errs = sorted(((rel(host(store.grad_of(k)), ref["grads"][k]), k) for k in store.live_keys
                   if np.linalg.norm(ref["grads"][k]) > 1e-4), reverse=True)
    med = np.median([e for e, _ in errs])
    print("bf16 loss", loss.item(), ref["loss"], "median", med, "worst", errs[:6])
    assert any("in_proj_weight" in k for _, k in errs) and any(".norm1." in k for _, k in errs)
    assert any("out_proj" in k for _, k in errs) and any("pos_embed" in k for _, k in errs)
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


def test_dropout_is_deterministic_per_seed_and_fresh_per_step():
    """vit_dropout = 0.1: two engines with the same seed agree bit for bit over three steps, another
    seed changes the loss, all values are finite."""
    batches = [make_multimodal_batch(B, G, L, 40 + s, with_originals=False) for s in range(3)]
    runs = {}
    for name, seed in (("a", 5), ("b", 5), ("c", 6)):
        _spec, store, eng, _ = build(vit_dropout=0.1, seed=seed)
        losses = torch.stack([eng.step(dev_batch(b)).clone() for b in batches]).cpu()
        runs[name] = (losses, store.student.clone().cpu(), store.teacher.clone().cpu())
    assert all(torch.equal(x, y) for x, y in zip(runs["a"], runs["b"]))
    assert not torch.equal(runs["a"][0], runs["c"][0])
    assert all(bool(torch.isfinite(t).all()) for r in runs.values() for t in r)
    _spec, _store, eng0, _ = build(vit_dropout=0.0, seed=5)
    l0 = eng0.step(dev_batch(batches[0])).item()
    assert l0 != runs["a"][0][0].item()                  # the masks act


def test_graph_dropout_masks_change_per_replay():
    """The same batch every step, with everything else frozen (lr 0, no weight decay, teacher and
    centre momentum 1): without dropout every step's loss is the same number; with vit_dropout the
    device seed offset gives every replay fresh masks, exactly as the eager steps draw them."""
    b = dev_batch(make_multimodal_batch(B, G, L, 55, with_originals=False))
    outs = {}
    for p, graph in ((0.0, True), (0.1, False), (0.1, True)):
        _spec, store, eng, _ = build(vit_dropout=p, seed=3)
        hp = eng.hp
        hp.lr, hp.wd, hp.momentum, hp.center_momentum = 0.0, 0.0, 1.0, 1.0
        eng.use_graph = graph
        outs[(p, graph)] = [eng.step(b).item() for _ in range(6)]
        assert eng.graph.captures == int(graph)
    print(outs)
    assert len(set(outs[(0.0, True)])) == 1
    assert outs[(0.1, False)] == outs[(0.1, True)]
    assert len(set(outs[(0.1, True)])) == 6 and all(np.isfinite(outs[(0.1, True)]))


def test_eval_features_match_the_fixture_including_the_ragged_batch():
    spec, store, eng, state = build(stats=True)
    fx = gu.load(VR.EVAL_NAME + "_f64")
    bound = max(1e-5, 3 * gu.rel_err(gu.load(VR.EVAL_NAME)["feat0"], fx["feat0"]))
    for i, n in enumerate(VR.EVAL_BATCHES):
        x = make_multimodal_batch(n, 1, 1, VR.EVAL_SEED + i)["audio"]
        xs = torch.from_numpy(np.ascontiguousarray(x.reshape(n, 112, 112, 1))).cuda()
        f = eng.enc.forward_eval(eng.ws, store, "ev", xs.reshape(-1), n)
        assert f.shape == (n, D)
        print("eval", i, rel(host(f), fx[f"feat{i}"]), "bound", bound)
        assert rel(host(f), fx[f"feat{i}"]) < bound, (i, rel(host(f), fx[f"feat{i}"]), bound)


def test_lightning_step_probe_and_knn_run():
    """One UniModalDINOLightning.training_step, the epoch-end probe and the kNN classifier over
    the new encoder: shapes and finite values only."""
    from avdino import downstream as DS
    from avdino.models import UNIMODAL_MODEL_MAP, UniModalDINOLightning
    m = UniModalDINOLightning(encoder_class=UNIMODAL_MODEL_MAP["spectrogram_vit"], output_dim=D,
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


def test_engine_refuses_a_batch_whose_activations_cannot_fit():
    """The activation footprint is checked against the device's free memory before anything is
    allocated (no recomputation: every layer's activations are kept)."""
    _spec, _store, eng, _ = build()
    assert eng.activation_bytes(768, 256) == pytest.approx(26.9e9, rel=0.01)     # the config's batch, 128
    free = torch.cuda.mem_get_info()[0]
    n = int(free // (4 * 197 * 512 * 16 * 4) * 3) + 8
    before = eng.ws.nbytes()
    with pytest.raises(MemoryError, match="smaller batch"):
        eng._check_memory(n, 8, True)
    assert eng.ws.nbytes() == before
