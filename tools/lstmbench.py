"""Time the LSTM recurrence kernels alone and the whole spectrogram_lstm training step, bf16,
on one MI355X.

    python tools/lstmbench.py [--reps 20] [--warmup 5] [--batches 64 1024] [--out FILE]

Three kinds of measurement, each in a fresh child process (its own HIP context and allocator)
under its own time limit; the parent stops at the first child of the project's own code that
fails:
  rec    avd_lstm_fwd (save = 1) and avd_lstm_bwd at H = 128, T = 196, N = (2 + 4 views) x B
         sequences: ms per launch, the time per step of the time loop (ms / T), saved-state bytes
         per sample;
  step   the graph-replayed UniModalEngine step, 2 + 4 views, D = 256, P = 128, for
         spectrogram_lstm and, as the yardstick, spectrogram_simple (one conv block more, no
         LSTM) at the same B;
  torch  torch.nn.LSTM forward + backward on the device at the rec shapes (bf16 and f32), the
         library path as a second yardstick.  This child may fail (no library kernels for the
         device): the parent then records that it did not run and goes on.
Every figure is the mean of HIP events around each of ``reps`` (>= 20) launches / replays after
``warmup`` untimed ones, with min and max."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, T, G, L, D, P = 128, 196, 2, 4, 256, 128


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


def child_rec(args):
    sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-ssl-avmnist_amd")]
    import torch
    from avdino import ops
    N = (G + L) * args.batch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    ns, ng = ops.lstm_ws(N, T, H)
    gx = torch.randn(ng, generator=g, device=dev)
    w = [(torch.rand(4 * H * H, generator=g, device=dev) * 2 - 1) / H ** 0.5 for _ in range(2)]
    out, save, dg = torch.empty(N * 2 * H, device=dev), torch.empty(ns, device=dev), torch.empty(ng, device=dev)
    dout = torch.randn(N * 2 * H, generator=g, device=dev)
    fwd = _timed(lambda: ops.lstm_fwd(gx, w[0], w[1], out, save, N, T, H, True), args.warmup, args.reps)
    fwd0 = _timed(lambda: ops.lstm_fwd(gx, w[0], w[1], out, None, N, T, H, True), args.warmup, args.reps)
    bwd = _timed(lambda: ops.lstm_bwd(dout, w[0], w[1], save, dg, N, T, H, True), args.warmup, args.reps)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dg).all())
    print(json.dumps({"what": "rec", "B": args.batch, "N": N, "T": T, "H": H, "fwd_save": fwd, "fwd_nosave": fwd0,
                      "bwd": bwd, "fwd_us_per_time_step": round(fwd["ms"] / T * 1e3, 3),
                      "bwd_us_per_time_step": round(bwd["ms"] / T * 1e3, 3),
                      "saved_bytes_per_sample": 4 * ns // N, "gx_bytes_per_sample": 4 * ng // N,
                      "workgroups": 2 * -(-N // ops.LSTM_BLOCK)}), flush=True)


def child_step(args):
    sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-ssl-avmnist_amd")]
    import torch
    from avdino.engine import Hyper, UniModalEngine
    from avdino.params import ParamStore
    from avdino.spec import unimodal_dino_sd
    dev = torch.device("cuda", 0)
    B = args.batch
    store = ParamStore(unimodal_dino_sd(args.model, D, P), dev, seed=0)
    eng = UniModalEngine(store, args.model, D, P, Hyper(), act_dtype=torch.bfloat16)
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
    print(json.dumps({"what": "step", "model": args.model, "B": B, "views": G + L, "step": r,
                      "samples_per_s": round(B / r["ms"] * 1e3, 1), "loss": round(lv, 5),
                      "workspace_GiB": round(eng.ws.nbytes() / 2 ** 30, 2)}), flush=True)


def child_torch(args):
    import torch
    N = (G + L) * args.batch
    dev = torch.device("cuda", 0)
    res = {"what": "torch", "B": args.batch, "N": N, "T": T, "H": H}
    for name, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        m = torch.nn.LSTM(64, H, batch_first=True, bidirectional=True).to(dev, dt)
        x = torch.randn(N, T, 64, device=dev, dtype=dt, requires_grad=True)

        def fb():
            m.zero_grad(set_to_none=True)
            x.grad = None
            m(x)[0].mean(dim=1).sum().backward()

        res[name + "_fwd_bwd"] = _timed(fb, 3, args.reps)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=None)
    ap.add_argument("--what", default=None, help="(child) rec | step | torch")
    ap.add_argument("--model", default="spectrogram_lstm", help="(child) the encoder of a step child")
    ap.add_argument("--batch", type=int, default=64, help="(child) B")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.what:
        return {"rec": child_rec, "step": child_step, "torch": child_torch}[args.what](args)
    # the project's own measurements first, the library yardstick last
    jobs = []
    for B in args.batches:
        jobs.append(("rec", None, B))
        jobs += [("step", m, B) for m in ("spectrogram_lstm", "spectrogram_simple")]
    jobs += [("torch", None, B) for B in args.batches]
    lines, torch_ok = [], True
    for what, model, B in jobs:
        if what == "torch" and not torch_ok:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--batch", str(B),
               "--reps", str(args.reps), "--warmup", str(args.warmup)] + (["--model", model] if model else [])
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            rc, tail = p.returncode, (p.stdout + p.stderr)[-600:]
            recs = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        except subprocess.TimeoutExpired:
            rc, tail, recs = "time limit", "", []
        if rc == 0 and recs:
            lines.append(recs[-1])
            print(lines[-1], flush=True)
            continue
        if what == "torch" and rc == 1:
            # an ordinary Python error (e.g. no library kernels for this device): say so, go on
            torch_ok = False
            last = (tail.strip().splitlines() or [""])[-1]
            lines.append(json.dumps({"what": "torch", "B": B, "ran": False, "tail": last[-300:]}))
            print(lines[-1], flush=True)
            continue
        # a failure of the project's own code, or any abort / signal / time limit: nothing more
        # is started on the device
        sys.stderr.write(tail)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        raise SystemExit(f"child {what}/{model}/B={B} failed with {rc}: stopping")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
