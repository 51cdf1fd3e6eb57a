"""spectrogram_vit with vit_attention="mfma" (avd_mhsa_mfma_*, csrc/mhsa_mfma.hip): the bf16 engine
step against the float64 restatement with the bands tests/test_gpu_uni_vit.py sets for the bf16
step, graph replay against eager steps, dropout determinism, the eval features, and the refusal of
the f32 parity mode.  Build and fixtures are those of tests/test_gpu_uni_vit.py; its ``build`` is
restated here with the ``vit_attention`` argument.

Eval features: no bf16 fixture exists, so the bound is 3 x the error the "exact" bf16 engine shows
against the same float64 fixture features in the same test (the project's usual factor on the
existing path's own error).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle.params import make_multimodal_batch  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import vit_ref as VR  # noqa: E402
from tests.test_gpu_uni_vit import B, D, G, HP, L, P, dev_batch, host, rel  # noqa: E402


def build(Dd=D, Pp=P, pseed=VR.PSEED, act=torch.bfloat16, stats=False, vit_dropout=0.0, seed=0,
          vit_attention="mfma"):
    from avdino.engine import Hyper, UniModalEngine
    from avdino.params import ParamStore
    spec = VR.vit_spec(Dd, Pp)
    store = ParamStore(spec, "cuda")
    state = VR.vit_state(spec, pseed, stats=stats)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    hp = Hyper(lr=HP["lr"], weight_decay=HP["wd"], momentum=HP["momentum"],
               center_momentum=HP["center_momentum"], student_temperature=HP["tau_s"],
               teacher_temperature=HP["tau_t"], dropout=0.0, fusion_dropout=0.0, vit_dropout=vit_dropout)
    eng = UniModalEngine(store, VR.KIND, Dd, Pp, hp, act_dtype=act, seed=seed, vit_attention=vit_attention)
    return spec, store, eng, state


def test_bf16_step_close_to_the_restatement():
    """The shape and bands of test_gpu_uni_vit.test_bf16_step_close_to_the_restatement; the
    difference to an "exact" engine on the same state and batch is printed."""
    Dd, Pp, Bb = 64, 32, 4
    batch = make_multimodal_batch(Bb, 2, 2, 3210, with_originals=False)
    spec, store, eng, state = build(Dd, Pp, 321)
    assert eng.enc.tower.attention == "mfma" and eng.t_enc.tower.attention == "mfma"
    ref = VR.unimodal_step(state, batch, HP, spec)
    loss = eng.forward(dev_batch(batch))
    eng.update_center()
    eng.backward()
    _spec, xstore, xeng, _ = build(Dd, Pp, 321, vit_attention="exact")
    xloss = xeng.forward(dev_batch(batch))
    xeng.update_center()
    xeng.backward()
    diff = sorted(((rel(host(store.grad_of(k)), host(xstore.grad_of(k))), k) for k in store.live_keys
                   if np.linalg.norm(ref["grads"][k]) > 1e-4), reverse=True)
    print("mfma loss", loss.item(), "exact loss", xloss.item(), "float64", ref["loss"])
    print("mfma vs exact gradients: median", np.median([e for e, _ in diff]), "worst", diff[:4])
    assert abs(loss.item() - ref["loss"]) < 2e-2 * abs(ref["loss"])
    errs = sorted(((rel(host(store.grad_of(k)), ref["grads"][k]), k) for k in store.live_keys
                   if np.linalg.norm(ref["grads"][k]) > 1e-4), reverse=True)
    med = np.median([e for e, _ in errs])
    print("bf16 mfma vs float64: median", med, "worst", errs[:6])
    assert any("in_proj_weight" in k for _, k in errs) and any(".norm1." in k for _, k in errs)
    assert any("out_proj" in k for _, k in errs) and any("pos_embed" in k for _, k in errs)
    assert med < 0.2 and errs[0][0] < 0.6, (med, errs[:6])


def test_graph_step_is_bitwise_the_eager_step():
    """Five steps: two eager warm-up steps, capture at the third, replays; all five losses and the
    state after them equal the eager engine's bit for bit."""
    batches = [make_multimodal_batch(B, G, L, 90 + s, with_originals=False) for s in range(5)]
    runs = []
    for graph in (False, True):
        _spec, store, eng, _ = build()
        eng.use_graph = graph
        losses = [eng.step(dev_batch(b)).clone() for b in batches]
        torch.cuda.synchronize()
        assert eng.graph.captures == (1 if graph else 0)
        runs.append((torch.stack(losses).cpu(), store.student.clone().cpu(), store.teacher.clone().cpu(),
                     store.buf_arena.clone().cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]).all()


def test_dropout_is_deterministic_per_seed():
    """vit_dropout = 0.1: two engines of one seed agree bit for bit over three steps, another seed
    differs, all values are finite."""
    batches = [make_multimodal_batch(B, G, L, 40 + s, with_originals=False) for s in range(3)]
    runs = {}
    for name, seed in (("a", 5), ("b", 5), ("c", 6)):
        _spec, store, eng, _ = build(vit_dropout=0.1, seed=seed)
        losses = torch.stack([eng.step(dev_batch(b)).clone() for b in batches]).cpu()
        runs[name] = (losses, store.student.clone().cpu(), store.teacher.clone().cpu())
    assert all(torch.equal(x, y) for x, y in zip(runs["a"], runs["b"]))
    assert not torch.equal(runs["a"][0], runs["c"][0])
    assert all(bool(torch.isfinite(t).all()) for r in runs.values() for t in r)


def test_eval_features_within_three_times_the_exact_bf16_error():
    fx = gu.load(VR.EVAL_NAME + "_f64")
    engines = {kind: build(stats=True, vit_attention=kind) for kind in ("exact", "mfma")}
    for i, n in enumerate(VR.EVAL_BATCHES):
        x = make_multimodal_batch(n, 1, 1, VR.EVAL_SEED + i)["audio"]
        xs = torch.from_numpy(np.ascontiguousarray(x.reshape(n, 112, 112, 1))).cuda().to(torch.bfloat16)
        err = {}
        for kind, (_spec, store, eng, _state) in engines.items():
            f = eng.enc.forward_eval(eng.ws, store, "ev", xs.reshape(-1), n)
            assert f.shape == (n, D)
            err[kind] = rel(host(f), fx[f"feat{i}"])
        print("eval", i, err, "bound", 3 * err["exact"])
        assert err["mfma"] <= 3 * err["exact"], (i, err)


def test_f32_activations_with_mfma_raise():
    with pytest.raises(ValueError, match="bf16"):
        build(act=torch.float32)
