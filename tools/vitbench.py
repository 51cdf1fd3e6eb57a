"""Time the ViT kernels alone and the whole spectrogram_vit training step, bf16, on one MI355X.

    python tools/vitbench.py [--reps 20] [--warmup 5] [--batch 128] [--rounds 2] [--out FILE]

Two kinds of measurement, each in a fresh child process (its own HIP context and allocator) under
its own time limit; the parent stops at the first child that fails:
  ops    at the model's shapes -- N = (2 + 4 views) x B sequences of T = 197 tokens, 4 heads of
         dh = 128, E = 512, F = 2048 -- ms per launch of avd_mhsa_fwd (with lse) / avd_mhsa_bwd,
         avd_ln_fwd (residual, saved state) / avd_ln_bwd and avd_gelu_fwd / avd_gelu_bwd; for the
         attention kernels the achieved FLOP/s (4 N heads T^2 dh forward, 10 N heads T^2 dh
         backward -- operations of the algorithm, computed here from the shapes) against the bf16
         MFMA peak and against the f32 vector rate the present kernels run at, and the time of
         the same problem through avd_xattn_fwd / avd_xattn_bwd, called per head with dirs = 1,
         groups = N, a zero x and scale = dh^-0.5 (the time of its four calls, summed); and, in
         the same process at the same shape, avd_mhsa_mfma_fwd / _bwd (p = 0 and p = 0.1) with
         the same FLOP formulas and their ratios to both;
  step   the graph-replayed UniModalEngine step, 2 + 4 views, D = 256, P = 128, for
         spectrogram_vit with --attention exact and mfma, alternating, ``--rounds`` times each (the
         repeated lines show the run-to-run spread), and, on the same box in the same run,
         spectrogram_simple and spectrogram_lstm at the same B.
Every figure is the mean of HIP events around each of ``reps`` (>= 20) launches / replays after
``warmup`` untimed ones, with min and max.  Lines are appended to ``--out``."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HEADS, DH, G, L, D, P = 197, 4, 128, 2, 4, 256, 128
E, F = HEADS * DH, 4 * HEADS * DH
PEAK_BF16_MFMA = 2516.8e12      # FLOP/s: 16 x the 157.3 TFLOP/s f32 matrix / vector rate
PEAK_F32_VALU = 157.3e12


def _timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = [s.elapsed_time(e) for s, e in ev]
    return {"ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def child_ops(args):
    sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-ssl-avmnist_amd")]
    import torch
    from avdino import ops
    N = (G + L) * args.batch
    R = N * T
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    qkv = torch.randn(R * 3 * E, generator=g, device=dev)
    do = torch.randn(R * E, generator=g, device=dev)
    ctx, lse = torch.empty(R * E, device=dev), torch.empty(N * HEADS * T, device=dev)
    dqkv = torch.empty(R * 3 * E, device=dev)
    aws = torch.empty(ops.mhsa_bwd_ws(N, HEADS, T, DH), device=dev)
    q, k, v = (qkv, 0, 3 * E), (qkv, E, 3 * E), (qkv, 2 * E, 3 * E)
    dq, dk, dv = (dqkv, 0, 3 * E), (dqkv, E, 3 * E), (dqkv, 2 * E, 3 * E)
    scale = DH ** -0.5
    res = {"what": "ops", "B": args.batch, "N": N, "T": T, "heads": HEADS, "dh": DH}
    w, r = args.warmup, args.reps
    for name, p in (("mhsa", 0.0), ("mhsa_drop0.1", 0.1)):
        res[name + "_fwd"] = _timed(lambda: ops.mhsa_fwd(q, k, v, (ctx, 0, E), lse, N, HEADS, T, DH, scale, True, p, 11),
                                    w, r)
        res[name + "_bwd"] = _timed(lambda: ops.mhsa_bwd((do, 0, E), q, k, v, lse, dq, dk, dv, aws, N, HEADS, T, DH,
                                                         scale, True, p, 11), w, r)
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(dqkv).all())
    mws = torch.empty(ops.mhsa_mfma_bwd_ws(N, HEADS, T, DH), device=dev)
    for name, p in (("mhsa_mfma", 0.0), ("mhsa_mfma_drop0.1", 0.1)):
        res[name + "_fwd"] = _timed(lambda: ops.mhsa_mfma_fwd(q, k, v, (ctx, 0, E), lse, N, HEADS, T, DH, scale, p, 11),
                                    w, r)
        res[name + "_bwd"] = _timed(lambda: ops.mhsa_mfma_bwd((do, 0, E), q, k, v, lse, dq, dk, dv, mws, N, HEADS, T,
                                                              DH, scale, p, 11), w, r)
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(dqkv).all())
    fl_f, fl_b = 4 * N * HEADS * T * T * DH, 10 * N * HEADS * T * T * DH
    for tag, fl in (("fwd", fl_f), ("bwd", fl_b)):
        for fam in ("mhsa", "mhsa_mfma"):
            rate = fl / (res[f"{fam}_{tag}"]["ms"] * 1e-3)
            res[f"{fam}_{tag}_tflops"] = round(rate / 1e12, 2)
            res[f"{fam}_{tag}_share_of_bf16_mfma_peak"] = round(rate / PEAK_BF16_MFMA, 4)
            if fam == "mhsa":
                res[f"mhsa_{tag}_share_of_f32_vector_rate"] = round(rate / PEAK_F32_VALU, 4)
    # the same problem through the cross-attention kernel: one call per head
    zero = torch.zeros(R * E, device=dev)
    xlse = torch.empty(HEADS, N * T, device=dev)
    xws = torch.empty(ops.xattn_bwd_ws(1, N, T, DH), device=dev)

    def xf():
        for h in range(HEADS):
            o = h * DH
            ops.xattn_fwd((qkv, o, 3 * E, 0), (qkv, E + o, 3 * E, 0), (qkv, 2 * E + o, 3 * E, 0), (zero, o, E, 0),
                          (ctx, o, E, 0), xlse[h], 1, N, T, DH, scale)

    def xb():
        for h in range(HEADS):
            o = h * DH
            ops.xattn_bwd((do, o, E, 0), (qkv, o, 3 * E, 0), (qkv, E + o, 3 * E, 0), (qkv, 2 * E + o, 3 * E, 0),
                          xlse[h], (dqkv, o, 3 * E, 0), (dqkv, E + o, 3 * E, 0), (dqkv, 2 * E + o, 3 * E, 0), xws, 1, N,
                          T, DH, scale)

    res["xattn_fwd_4_heads"] = _timed(xf, w, r)
    res["xattn_bwd_4_heads"] = _timed(xb, w, r)
    res["mhsa_over_xattn_fwd"] = round(res["mhsa_fwd"]["ms"] / res["xattn_fwd_4_heads"]["ms"], 2)
    res["mhsa_over_xattn_bwd"] = round(res["mhsa_bwd"]["ms"] / res["xattn_bwd_4_heads"]["ms"], 2)
    for tag in ("fwd", "bwd"):
        res[f"mhsa_mfma_over_xattn_{tag}"] = round(res[f"mhsa_mfma_{tag}"]["ms"] / res[f"xattn_{tag}_4_heads"]["ms"], 4)
        res[f"mhsa_over_mhsa_mfma_{tag}"] = round(res[f"mhsa_{tag}"]["ms"] / res[f"mhsa_mfma_{tag}"]["ms"], 2)
    # LayerNorm and GELU at the model's row counts
    x, rr, y, z = (torch.randn(R * E, generator=g, device=dev) for _ in range(4))
    gam, bet = torch.ones(E, device=dev), torch.zeros(E, device=dev)
    mean, rstd = torch.empty(R, device=dev), torch.empty(R, device=dev)
    dx, dr, dg, db = torch.empty(R * E, device=dev), torch.empty(R * E, device=dev), torch.empty(E, device=dev), \
        torch.empty(E, device=dev)
    lws = torch.empty(ops.ln_bwd_ws(R, E), device=dev)
    res["ln_fwd"] = _timed(lambda: ops.ln_fwd(x, rr, gam, bet, y, R, E, z, mean, rstd, 1e-5, 0.1, 5), w, r)
    res["ln_bwd"] = _timed(lambda: ops.ln_bwd(do, z, mean, rstd, gam, dx, dr, dg, db, lws, R, E, 0.1, 5), w, r)
    res["ln_fwd_GBps"] = round(4 * 4 * R * E / (res["ln_fwd"]["ms"] * 1e-3) / 1e9, 1)
    res["ln_bwd_GBps"] = round(4 * 4 * R * E / (res["ln_bwd"]["ms"] * 1e-3) / 1e9, 1)
    f1, f2 = torch.randn(R * F, generator=g, device=dev), torch.empty(R * F, device=dev)
    res["gelu_fwd"] = _timed(lambda: ops.gelu_fwd(f1, f2, R, F, 0.1, 5), w, r)
    res["gelu_bwd"] = _timed(lambda: ops.gelu_bwd(f1, f2, f2, R, F, 0.1, 5), w, r)
    res["gelu_fwd_GBps"] = round(2 * 4 * R * F / (res["gelu_fwd"]["ms"] * 1e-3) / 1e9, 1)
    res["gelu_bwd_GBps"] = round(3 * 4 * R * F / (res["gelu_bwd"]["ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(res), flush=True)


def child_step(args):
    sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-ssl-avmnist_amd")]
    import torch
    from avdino.engine import Hyper, UniModalEngine
    from avdino.params import ParamStore
    from avdino.spec import unimodal_dino_sd
    dev = torch.device("cuda", 0)
    B = args.batch
    store = ParamStore(unimodal_dino_sd(args.model, D, P), dev, seed=0)
    if args.model == "spectrogram_vit":      # torch's zero cls / position tokens would make every
        gen0 = torch.Generator().manual_seed(3)     # token of a noise image alike
        for k in ("cls_token", "pos_embed"):
            t = store[f"student.encoder.0.{k}"]
            t.copy_(torch.randn(t.shape, generator=gen0) * 0.02)
            store[f"teacher.encoder.0.{k}"].copy_(t)
    eng = UniModalEngine(store, args.model, D, P, Hyper(), act_dtype=torch.bfloat16, vit_attention=args.attention)
    eng.use_graph = True
    gen = torch.Generator(device=dev).manual_seed(1234)

    def px(*shape):
        return torch.randint(0, 256, shape, generator=gen, device=dev, dtype=torch.int32).float() / 255.0

    pool = [{"g_aud": px(B, G, 1, 112, 112), "l_aud": px(B, L, 1, 112, 112)} for _ in range(2)]
    i = [0]

    def step():
        i[0] += 1
        return eng.step(pool[i[0] % 2])

    r = _timed(step, max(args.warmup, 4), args.reps)
    assert len(eng.graph.graphs) == 1, "the timed steps must be graph replays"
    lv = float(eng.last["loss"].item())
    assert lv == lv, "loss is NaN"
    print(json.dumps({"what": "step", "model": args.model, "attention": args.attention, "B": B, "views": G + L,
                      "step": r,
                      "samples_per_s": round(B / r["ms"] * 1e3, 1), "loss": round(lv, 5),
                      "workspace_GiB": round(eng.ws.nbytes() / 2 ** 30, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128, help="B (the config's batch size)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--what", default=None, help="(child) ops | step")
    ap.add_argument("--model", default="spectrogram_vit", help="(child) the encoder of a step child")
    ap.add_argument("--attention", default="exact", choices=["exact", "mfma"],
                    help="(child) the ViT attention kernels of a step child")
    ap.add_argument("--rounds", type=int, default=2, help="exact / mfma spectrogram_vit step pairs")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.what:
        return {"ops": child_ops, "step": child_step}[args.what](args)
    jobs = [("ops", None, None)]
    jobs += [("step", "spectrogram_vit", att) for _ in range(max(args.rounds, 1)) for att in ("exact", "mfma")]
    jobs += [("step", m, "exact") for m in ("spectrogram_simple", "spectrogram_lstm")]
    for what, model, att in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--batch", str(args.batch),
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        cmd += ["--model", model, "--attention", att] if model else []
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            rc, tail = p.returncode, (p.stdout + p.stderr)[-800:]
            recs = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        except subprocess.TimeoutExpired:
            rc, tail, recs = "time limit", "", []
        if rc == 0 and recs:
            print(recs[-1], flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(recs[-1] + "\n")
            continue
        # any failure, abort, signal or time limit: nothing more is started on the device
        sys.stderr.write(tail)
        raise SystemExit(f"child {what}/{model}/{att} failed with {rc}: stopping")


if __name__ == "__main__":
    main()
