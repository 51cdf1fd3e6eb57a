"""Time the eval-mode forward (ConvBranch.forward_eval, bf16) of the two SimCLR encoders, whole
and per layer, with HIP events.
    python tools/evalbench.py [--tree PATH] [--n 128,1024] [--rounds 3] [--fused 1|0]

--tree selects the checkout whose package and library are timed (default: this one), so the
same script times a parent build next to the new one: run the two alternately, a few rounds each,
on one box, and compare per layer against the spread of the rounds.  --fused 0 turns
ConvBranch.EVAL_FUSED off where the tree has it (the cross-check that the two-launch route did
not move); a tree without the attribute only has the two-launch route.

Per layer = the launches of one conv block (conv + pool, or the one fused launch), each replayed
alone from the closures a KernelTimer pass records; whole = forward_eval end to end (weight
layouts and BN coefficients included).  One line per (encoder, N, round)."""
import argparse
import os
import sys
from collections import OrderedDict

import torch

LAYER_STARTS = ("cl_conv_fwd", "c3_conv_eval", "cl_c1_recompute", "c1r5_apply", "mx_conv_fwd")
LAYER_PARTS = LAYER_STARTS + ("cl_bn_relu_pool",)


def timeit(fn, n):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--n", default="128,1024")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused", type=int, default=1)
    ap.add_argument("--tag", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "multimodal-ssl-avmnist_amd")]
    from avdino import ops
    from avdino.engine import ConvBranch, Workspace
    from avdino.params import ParamStore
    from avdino.spec import CNN3_AUDIO_CONVS, CNN3_IMAGE_CONVS, _cnn3, cnn3_stack

    has = hasattr(ConvBranch, "EVAL_FUSED")
    if has:
        ConvBranch.EVAL_FUSED = bool(args.fused)
    route = "fused" if has and args.fused else "two-launch"
    tag = args.tag or os.path.basename(tree)
    T = torch.bfloat16
    for name, convs, hw in (("image", CNN3_IMAGE_CONVS, 28), ("audio", CNN3_AUDIO_CONVS, 112)):
        sd = OrderedDict()
        _cnn3(sd, "e.encoder", convs, 64)
        store = ParamStore(sd, "cuda", seed=1, has_teacher=False)
        br = ConvBranch(cnn3_stack("e.encoder", convs, hw), T)
        for N in [int(v) for v in args.n.split(",")]:
            x = torch.rand(N, hw, hw, 1, device="cuda").to(T)
            ws = Workspace(store.device)
            run = lambda: br.forward_eval(ws, store, "ev", x, N)  # noqa: E731
            run()
            ops.TIMER = ops.KernelTimer()
            run()
            fns = ops.TIMER.fns
            ops.TIMER = None
            layers = []
            for key, (fn, _nb, _fl) in fns.items():
                if key.startswith(LAYER_STARTS):
                    layers.append([])
                if layers and key.startswith(LAYER_PARTS):
                    layers[-1].append((key, fn))
            for r in range(args.rounds):
                whole = timeit(run, 20)
                per = [sum(timeit(fn, 20) for _k, fn in lay) for lay in layers]
                cells = "  ".join(f"L{i} {t:7.1f}" for i, t in enumerate(per))
                print(f"{tag} {route:10s} {name} N={N:5d} round {r}: whole {whole:8.1f} us  "
                      f"layers {sum(per):8.1f} us  {cells}", flush=True)
            if N == 128:
                print(f"{tag} {route:10s} {name} launches: " +
                      " | ".join("+".join(k.split("[")[0] for k, _ in lay) for lay in layers), flush=True)


if __name__ == "__main__":
    main()
