"""The gated and cross-attention fusion encoders (``--model multi_simple_gated`` /
``multi_cross_attention``) on the engine, against the REFERENCE's own float64 runs
(tests/golden/gen_fusion_golden.py: GatedMultiModalEncoder, CrossAttentionMultiModalEncoder).

fp32 engine mode, bands of test_gpu_step.py::test_simple_encoder_step_matches_reference for the
same towers: loss 3e-5 abs, outputs / centre rel-L2 1e-5, gradients 1e-3 with the audio tower at
1.5x the reference's own fp32-vs-float64 error (read from the new fixtures here), EMA'd teacher
1e-6, running statistics 1e-5; the free-running 3-step loss curve within test_gpu_step's
3e-5 on step 1 and 1e-3 after (Adam turns rounding noise on near-zero gradients into +-lr steps;
the reference's own fp32 run is 2.8e-4 off its float64 run by step 3 of mm_xattn_mse_small).

bf16 mode: the fused attention route against the plain route (which the fp32 test pins to the
reference) on one engine's state, within the computed bf16 rounding band (3x the float64 model
of the kernel's roundings, see test_gpu_xattn.py); graph replay == eager, bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle.params import make_multimodal_batch  # noqa: E402
from tests import fusion_util as FU  # noqa: E402
from tests import golden_util as gu  # noqa: E402

HP = dict(lr=1e-4, wd=1e-6, momentum=0.996, center_momentum=0.9, tau_s=0.1, tau_t=0.04)


def rel(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def dev_batch(b):
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}


def build(encoder, mode, E, D, P, pseed, act=torch.float32, dropout=0.0, seed=0):
    from avdino.engine import Hyper, MultiCentralEngine
    from avdino.params import ParamStore
    spec = FU.fusion_spec(mode, E, D, P, encoder)
    store = ParamStore(spec, "cuda")
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in FU.fusion_state(spec, pseed).items()})
    hp = Hyper(lr=HP["lr"], weight_decay=HP["wd"], momentum=HP["momentum"],
               center_momentum=HP["center_momentum"], student_temperature=HP["tau_s"],
               teacher_temperature=HP["tau_t"], dropout=dropout, fusion_dropout=dropout)
    return store, MultiCentralEngine(store, mode, E, D, P, hp, act_dtype=act, encoder=encoder, seed=seed)


def ref_fp32_audio_err(case, prefix="grad/student.audio_encoder"):
    """Worst rel-L2 error of the reference's own fp32 run against its float64 run over the
    audio-tower gradients of this fixture (fully stored tensors)."""
    f32, f64 = gu.load(case), gu.load(case + "_f64")
    worst = 0.0
    for k in f64:
        if k.startswith(prefix) and "@" not in k:
            b = np.asarray(f64[k], np.float64).ravel()
            if np.linalg.norm(b) > 1e-9:
                worst = max(worst, rel(f32[k], b))
    return worst


MIX_KEYS = {"multi_simple_gated": ["student.gate_image", "student.gate_audio"],
            "multi_cross_attention": [f"student.{a}.{p}.{w}" for a in ("image_to_audio_attention",
                                                                      "audio_to_image_attention")
                                      for p in ("q_proj", "kv_proj") for w in ("weight", "bias")]}


@pytest.mark.parametrize("case", list(FU.CASES))
def test_fusion_step_matches_reference(case):
    from avdino.engine import ema_step
    encoder, mode = FU.CASES[case]
    fx = gu.load(case + "_f64")
    E, D, P, B, G, L, pseed, bseed = [int(x) for x in fx["meta_dims"]]
    assert B == 5 and str(fx["meta_encoder"]) == encoder
    store, eng = build(encoder, mode, E, D, P, pseed)
    loss = eng.forward(dev_batch(make_multimodal_batch(B, G, L, bseed)))
    s_out, t_out = eng.outputs()
    print(case, "loss", loss.item(), "reference", float(fx["loss"]))
    assert abs(loss.item() - float(fx["loss"])) < 3e-5, (loss.item(), float(fx["loss"]))
    for k, v in (("s_out", s_out), ("t_out", t_out)):
        ok, msg = gu.compare(fx, k, host(v), rel=1e-5)
        print(msg)
        assert ok, msg
    eng.update_center()
    assert rel(host(store["center"]), fx["center_after"]) < 1e-5
    ema_step(store, HP["momentum"])
    eng.backward()
    zero = gu.zero_grad_keys(fx)
    live = [str(k) for k in fx["live_keys"]]
    assert sorted(live) == sorted(store.live_keys)
    audio_tol = max(1e-3, 1.5 * ref_fp32_audio_err(case))
    errs = {}
    for k in live:
        g = host(store.grad_of(k))
        if "grad/" + k in zero:
            assert np.linalg.norm(g) <= 1e-4, (k, np.linalg.norm(g))
            continue
        bound = audio_tol if k.startswith("student.audio_encoder") else 1e-3
        ok, msg = gu.compare(fx, "grad/" + k, g, rel=bound)
        assert ok, msg
        if "grad/" + k in fx:
            errs[k] = rel(g, fx["grad/" + k])
    print("worst grad rel errors:", sorted(errs.items(), key=lambda kv: -kv[1])[:5], "audio bound", audio_tol)
    assert np.median(list(errs.values())) < 1e-4
    # the mix stage's own parameters: present, live, non-zero, and right
    for k in MIX_KEYS[encoder]:
        assert k in live and np.linalg.norm(host(store.grad_of(k))) > 0, k
        print(k, "grad rel err", errs[k])
    for k in store.t_offs:
        ok, msg = gu.compare(fx, "ema/" + k, host(store[k]), rel=1e-6)
        assert ok, msg
    n_rs = 0
    for k in store.buffers:
        if k.endswith("running_mean") or k.endswith("running_var"):
            ok, msg = gu.compare(fx, "rs/" + k, host(store.buffers[k]), rel=1e-5)
            assert ok, msg
            n_rs += 1
    assert n_rs >= 2 * 2 * 7            # both statistics of the 3 + 4 tower BatchNorms, student and teacher


@pytest.mark.parametrize("case", list(FU.CASES))
def test_fusion_loss_curve_matches_reference(case):
    encoder, mode = FU.CASES[case]
    fx = gu.load(case + "_f64")
    E, D, P, B, G, L, pseed, bseed = [int(x) for x in fx["meta_dims"]]
    ref = np.asarray(fx["curve"])
    assert len(ref) == FU.STEPS == 3
    store, eng = build(encoder, mode, E, D, P, pseed)
    curve = [eng.step(dev_batch(make_multimodal_batch(B, G, L, bseed + s))).item() for s in range(len(ref))]
    print(case, "engine", curve, "reference f64", ref.tolist(), "diff", (np.array(curve) - ref).tolist())
    np.testing.assert_allclose(curve[:1], ref[:1], atol=3e-5, rtol=0)
    np.testing.assert_allclose(curve, ref, atol=1e-3, rtol=0)


# ---------------------------------------------------------------- bf16: fused vs plain route
def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _attn64(q, k, v, x, do, scale, rounded):
    """float64 attention of [groups, B, E] operands -> OUT, dQ, dK, dV (test_gpu_xattn.py's model)."""
    if rounded:
        q, k, v, do = _bf(q), _bf(k), _bf(v), _bf(do)
    p = (scale * q @ k.transpose(1, 2)).softmax(-1)
    dp = do @ v.transpose(1, 2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    pr, dsr = (_bf(p), _bf(ds)) if rounded else (p, ds)
    return x + pr @ v, scale * dsr @ k, scale * dsr.transpose(1, 2) @ q, pr.transpose(1, 2) @ do


FUSED_ROUTE_CASES = [(32, 5), (128, 70), (256, 70), (64, 17)]     # (256, 70): the configured size


@pytest.mark.parametrize("E,B", FUSED_ROUTE_CASES)
def test_bf16_fused_route_matches_plain_route(E, B):
    """One engine, one state: the mix stage forward and backward by the fused kernel and by the
    plain route, from the same cat and the same gradient of fusion's input."""
    from avdino.engine import XATTN_NAMES
    V, D, P = 3, 32, 16
    store, eng = build("multi_cross_attention", "mse", E, D, P, 77, act=torch.bfloat16)
    rows, N = V * B, (V + 1) * B
    g = torch.Generator().manual_seed(E + B)
    cat = (torch.randn(N * 2 * E, generator=g) * 4.0).cuda()
    dmix = torch.randn(N * 2 * E, generator=g).cuda()
    keys = MIX_KEYS["multi_cross_attention"]
    res = {}
    for fused in (True, False):
        eng.XATTN_FUSED = fused
        assert eng._xattn_fused() == fused
        store.grad.zero_()
        mix, mctx = eng._mix_fwd("student", cat, V, B, "s", train=True)
        dcat = dmix.clone()
        eng._mix_bwd(mctx, cat, dcat, V, B)
        torch.cuda.synchronize()
        res[fused] = dict(mix=host(mix).reshape(rows, 2 * E), dcat=host(dcat).reshape(N, 2 * E),
                          qkv=mctx[0].detach().double().cpu().reshape(2, rows, 3 * E),
                          grads={k: host(store.grad_of(k)) for k in keys})
    assert np.array_equal(res[True]["qkv"].numpy(), res[False]["qkv"].numpy())     # same projections
    assert np.array_equal(res[True]["dcat"][rows:], host(dmix).reshape(N, 2 * E)[rows:])   # originals' rows
    # the band: float64 with and without the kernel's roundings, from the engine's own Q, K, V
    qkv = res[False]["qkv"]
    c64 = cat.double().cpu().reshape(N, 2 * E)[:rows]
    d64 = dmix.double().cpu().reshape(N, 2 * E)[:rows]
    scale = E ** -0.5
    W = {k: store[k].detach().double().cpu() for k in keys}

    def downstream(rounded):
        out = {"mix": torch.empty(rows, 2 * E, dtype=torch.float64), "dcat": d64.clone()}
        for d, att in enumerate(XATTN_NAMES):
            q, k, v = (qkv[d][:, c * E:(c + 1) * E].reshape(V, B, E) for c in range(3))
            x = c64[:, d * E:(d + 1) * E].reshape(V, B, E)
            do = d64[:, d * E:(d + 1) * E].reshape(V, B, E)
            o, dq, dk, dv = (t.reshape(rows, E) for t in _attn64(q, k, v, x, do, scale, rounded))
            out["mix"][:, d * E:(d + 1) * E] = o
            dkv = torch.cat([dk, dv], 1)
            key = f"student.{att}"
            xq, xkv = c64[:, d * E:(d + 1) * E], c64[:, (1 - d) * E:(2 - d) * E]
            out["dcat"][:, d * E:(d + 1) * E] += dq @ W[key + ".q_proj.weight"]
            out["dcat"][:, (1 - d) * E:(2 - d) * E] += dkv @ W[key + ".kv_proj.weight"]
            out[key + ".q_proj.weight"], out[key + ".q_proj.bias"] = dq.T @ xq, dq.sum(0)
            out[key + ".kv_proj.weight"], out[key + ".kv_proj.bias"] = dkv.T @ xkv, dkv.sum(0)
        return out

    exact, model = downstream(False), downstream(True)
    got = {True: {}, False: {}}
    for f in (True, False):
        got[f] = dict(res[f]["grads"], mix=res[f]["mix"], dcat=res[f]["dcat"][:rows])
    for name in ["mix", "dcat"] + keys:
        bound = 3.0 * rel(model[name].numpy(), exact[name].numpy())
        err = rel(got[True][name], got[False][name])
        print(f"bf16 E{E} B{B} {name}: fused vs plain rel-L2 {err:.3e} (bound {bound:.3e}); plain vs float64 "
              f"{rel(got[False][name], exact[name].numpy()):.3e}")
        assert err <= bound, (name, err, bound)


def _run(encoder, graph, pipeline=False, steps=5):
    E, D, P, B, G, L = 32, 32, 16, 8, 2, 4
    store, eng = build(encoder, "mse", E, D, P, 403, act=torch.bfloat16, dropout=0.3, seed=3)
    eng.use_graph, eng.pipeline = graph, pipeline
    batches = [dev_batch(make_multimodal_batch(B, G, L, 4500 + i)) for i in range(2)]
    losses = [eng.step(batches[i % 2], next_batch=batches[(i + 1) % 2] if pipeline else None).item()
              for i in range(steps)]
    return store, losses, eng


@pytest.mark.parametrize("encoder", list(FU.ENCODERS))
def test_graph_replay_equals_eager(encoder):
    s0, l0, e0 = _run(encoder, False)
    s1, l1, e1 = _run(encoder, True)
    if encoder == "multi_cross_attention":
        assert e0._xattn_fused() and e1._xattn_fused()
    assert len(e1.graph.graphs) == 1
    assert l0 == l1, (l0, l1)
    assert len(set(l1)) > 1 and all(np.isfinite(l1))
    assert torch.equal(s0.student, s1.student) and torch.equal(s0.teacher, s1.teacher)
    assert torch.equal(s0.buf_arena, s1.buf_arena)
    assert torch.equal(s0.adam_m, s1.adam_m) and torch.equal(s0.adam_v, s1.adam_v)


def test_pipelined_teacher_equals_sequential_cross_attention():
    """The teacher-ahead path runs the same mix stage: losses and parameters of the sequential
    step, bit for bit (captured graph)."""
    s0, l0, _ = _run("multi_cross_attention", True, steps=6)
    s1, l1, e1 = _run("multi_cross_attention", True, pipeline=True, steps=6)
    assert l0 == l1, (l0, l1)
    assert torch.equal(s0.student, s1.student) and torch.equal(s0.teacher, s1.teacher)
    assert e1._t_ready is not None


# ---------------------------------------------------------------- eval / downstream
def _labelled(n_batches, B, last, seed):
    out = []
    for i in range(n_batches):
        n = last if i == n_batches - 1 else B
        b = make_multimodal_batch(n, 1, 1, seed + i)
        out.append((torch.from_numpy(b["image"]).cuda(), torch.from_numpy(b["audio"]).cuda(),
                    torch.from_numpy(b["label"]).cuda()))
    return out


def test_eval_features_match_reference_ragged_batch():
    """Eval-mode student features of two loader batches (6 and 3 samples): each call attends
    across its own batch, so the 3-sample batch is a ragged group of its own."""
    from avdino.probe import LinearProbe
    fx = gu.load(FU.EVAL_NAME + "_f64")
    E, D, P, pseed, eseed = [int(x) for x in fx["meta_dims"]]
    store, _eng = build("multi_cross_attention", "mse", E, D, P, pseed)
    probe = LinearProbe(store, "multi_cross_attention", D, E, act_dtype=torch.float32)
    for i, n in enumerate(int(x) for x in fx["meta_batches"]):
        b = make_multimodal_batch(n, 1, 1, eseed + i)
        feat = probe._features(torch.from_numpy(b["image"]).cuda(), torch.from_numpy(b["audio"]).cuda(), False)
        e = rel(host(feat).reshape(n, D), fx[f"feat{i}"])
        print(f"eval batch {i} ({n} samples): rel-L2 {e:.3e}")
        assert e < 1e-5, (i, e)


@pytest.mark.parametrize("precision", ["32", "bf16"])
def test_knn_and_linear_probe_run_on_cross_attention(precision):
    from avdino.downstream import train_knn_classifier
    from avdino.models import CrossAttentionMultiModalEncoder, MultiModalDINOWithMSE
    from avdino.probe import LinearProbe
    E = D = 32
    m = MultiModalDINOWithMSE(encoder_class=CrossAttentionMultiModalEncoder, output_dim=D,
                              encoder_output_dim=E, projection_dim=16, precision=precision, device="cuda")
    train, test = _labelled(3, 16, 7, 6300), _labelled(2, 16, 5, 6400)
    _knn, acc = train_knn_classifier(m, train, test, n_neighbors=3)
    assert 0.0 <= acc <= 100.0
    act = torch.bfloat16 if precision == "bf16" else torch.float32
    probe = LinearProbe(m.store, "multi_cross_attention", D, E, act_dtype=act)
    r = probe.run_epoch(train, test)
    assert np.isfinite(r["val_loss"]) and np.isfinite(r["eval_loss"]) and 0.0 <= r["mlp_acc"] <= 100.0
    assert bool(torch.isfinite(r["logits"]).all())


@pytest.mark.parametrize("model", list(FU.ENCODERS))
def test_run_dino_trains_on_device(model, capsys):
    """The driver end to end on the new encoders: 3 steps, the epoch-end probe, finite losses."""
    import json
    import os

    from avdino import run_dino as R
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                       "config_multimodal_dino.yaml")
    m = R.main(["--model", model, "--training_mode", "mse", "--config", cfg, "--epochs", "1",
                "--steps-per-epoch", "3", "--batch-size", "8", "--probe-batches", "2", "--synthetic",
                "--seeds", "1"])
    recs = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(recs) == 1 and np.isfinite(recs[0]["train_loss"]) and 0 <= recs[0]["mlp_acc"] <= 100
    assert m.model.engine.step_idx == 3 and m.model.engine.mix is not None
