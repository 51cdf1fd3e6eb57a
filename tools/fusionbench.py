"""Time the bf16 graph-replayed training step of the three 3x3-tower fusion encoders --
multi_simple, multi_simple_gated, multi_cross_attention -- at the bench shape (B = 1024, 2 + 4
views, E = D = 256, P = 128, mse mode), and A/B the two cross-attention routes: the fused
avd_xattn_fwd / avd_xattn_bwd kernels against the plain avd_gemm + row-softmax route
(MultiCentralEngine.XATTN_FUSED).

    python tools/fusionbench.py [--runs 5] [--steps 30] [--warmup 6] [--batch 1024] [--out FILE]

Every measurement is a fresh child process (its own HIP context, allocator and graph capture);
the configurations run alternating, round by round, on the same device, so drift hits all of
them alike.  Per configuration: every run's ms/step and the median.  The parent stops at the
first child that fails.  bench.py stays the flagship yardstick; this tool only compares the
fusion kinds with each other."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("multi_simple", "-"), ("multi_simple_gated", "-"), ("multi_cross_attention", "fused"),
           ("multi_cross_attention", "plain")]


def child(args):
    sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-ssl-avmnist_amd")]
    import torch
    from avdino import ops
    from avdino.engine import Hyper, MultiCentralEngine
    from avdino.params import ParamStore
    from avdino.spec import multimodal_dino_sd
    dev = torch.device("cuda", 0)
    E, D, P, G, L, B = 256, 256, 128, 2, 4, args.batch
    store = ParamStore(multimodal_dino_sd("mse", E, D, P, encoder=args.model), dev, seed=0)
    eng = MultiCentralEngine(store, "mse", E, D, P, Hyper(), act_dtype=torch.bfloat16, encoder=args.model)
    if args.route != "-":
        eng.XATTN_FUSED = args.route == "fused"
    eng.use_graph = True
    gen = torch.Generator(device=dev).manual_seed(1234)

    def px(*shape):
        return torch.randint(0, 256, shape, generator=gen, device=dev, dtype=torch.int32).float() / 255.0

    pool = [{"g_img": px(B, G, 1, 28, 28), "g_aud": px(B, G, 1, 112, 112), "l_img": px(B, L, 1, 28, 28),
             "l_aud": px(B, L, 1, 112, 112), "image": px(B, 1, 28, 28), "audio": px(B, 1, 112, 112),
             "label": torch.randint(0, 10, (B,), generator=gen, device=dev)} for _ in range(2)]
    # library entry-point calls of one eager step (each is one launch, a few are two or three)
    calls, real = [0], ops.call

    def counting(name, *a):
        calls[0] += 1
        return real(name, *a)

    for i in range(args.warmup):
        ops.call = counting if i == 1 else real
        loss = eng.step(pool[i % 2])
    ops.call = real
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = eng.step(pool[i % 2])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    assert len(eng.graph.graphs) == 1, "the timed steps must be graph replays"
    lv = float(loss.item())
    assert lv == lv, "loss is NaN"
    print(json.dumps({"model": args.model, "route": args.route, "ms_per_step": round(ms, 4),
                      "pairs_per_s": round(B / ms * 1e3, 1), "loss": round(lv, 5), "B": B,
                      "steps": args.steps, "entry_calls_per_step": calls[0]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default=None, help="(child) the encoder to time")
    ap.add_argument("--route", default="-", help="(child) fused | plain | -")
    args = ap.parse_args()
    if args.model:
        return child(args)
    res = {c: [] for c in CONFIGS}
    lines = []
    for r in range(args.runs):
        for model, route in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--model", model, "--route", route,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"child {model}/{route} failed with {p.returncode}: stopping")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            rec["round"] = r
            res[(model, route)].append(rec["ms_per_step"])
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    base = statistics.median(res[CONFIGS[0]])
    for (model, route), v in res.items():
        med = statistics.median(v)
        lines.append(json.dumps({"summary": model, "route": route, "runs": len(v), "median_ms": round(med, 4),
                                 "min_ms": min(v), "max_ms": max(v),
                                 "median_pairs_per_s": round(args.batch / med * 1e3, 1),
                                 "vs_multi_simple": round(med / base, 4)}))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
