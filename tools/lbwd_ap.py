"""One fused layer backward alone at config-2 size, with the BN-backward apply in the kernel
recomputing the pool's argmax (y + pooled gradient, AP = 1), routed by the forward pool's codes
(AP = 2), and with a precomputed dY (AP = 0): how much of the launch is the apply; the three
launches it replaces (apply, input gradient, weight gradient), each alone, and their sum; and the
forward pool with and without the code stores.
    python tools/lbwd_ap.py [--layer 56|28] [--n N] [--b B]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-ssl-avmnist_amd")]
import torch  # noqa: E402

from avdino import ops  # noqa: E402

LAYERS = {56: (8, 56, 16), 28: (16, 28, 32)}     # input map: (Cin, H, Cout), 5x5 pad 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", type=int, choices=sorted(LAYERS), default=56,
                    help="input map of the layer: 56 = audio conv2 (8 -> 16), 28 = audio conv3 (16 -> 32)")
    ap.add_argument("--n", type=int, default=7168)
    ap.add_argument("--b", type=int, default=1024)
    a = ap.parse_args()
    N, B, K, pad = a.n, a.b, 5, 2
    Cin, H, Cout = LAYERS[a.layer]
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = torch.bfloat16

    def rnd(*s, dt=bf):
        return (torch.rand(*s, generator=g, device="cuda") * 2 - 1).to(dt)
    x = rnd(N * H * H * Cin)
    y = rnd(N * H * H * Cout)
    gout = rnd(N * (H // 2) * (H // 2) * Cout)
    dy = rnd(N * H * H * Cout)
    G = N // B
    scale = torch.rand(G * Cout, device="cuda") + 0.5
    shift = torch.rand(G * Cout, device="cuda") - 0.5
    coef = torch.rand(G * Cout * 3, device="cuda")
    w = torch.randn(Cout, Cin, K, K, device="cuda") * 0.1
    wk = torch.empty(ops.cl_weight_elems(Cout, Cin, K, 1), dtype=bf, device="cuda")
    ops.cl_weight_layout(w, wk, 1)
    slabs = ops.cl_layer_bwd_slabs(bf, N, Cin, H, H, Cout, K, pad)
    parts = torch.empty(slabs * Cout * Cin * K * K, device="cuda")
    nch = ops.cl_wgrad_chunks(N, Cout, Cin, K)
    wparts = torch.empty(nch * Cout * Cin * K * K, device="cuda")
    dx = torch.empty_like(x)
    dy2 = torch.empty_like(dy)
    pooled = torch.empty_like(gout)
    codes = torch.empty(gout.numel() // 8, dtype=torch.int32, device="cuda")
    ops.cl_bn_relu_pool_codes(y, scale, shift, pooled, codes, N, B, Cout, H, H)
    print(f"layer {H}x{H} {Cin}->{Cout}, N={N} B={B}: {slabs} slabs", flush=True)
    runs = {"apply (AP=1)": lambda: ops.cl_layer_bwd(y, gout, scale, shift, coef, None, x, wk, dx, parts, slabs,
                                                     N, B, Cin, H, H, Cout, K, pad),
            "apply from codes (AP=2)": lambda: ops.cl_layer_bwd(y, gout, scale, shift, coef, None, x, wk, dx, parts,
                                                                slabs, N, B, Cin, H, H, Cout, K, pad, codes=codes),
            "dY given (AP=0)": lambda: ops.cl_layer_bwd(None, None, None, None, None, dy, x, wk, dx, parts, slabs,
                                                        N, B, Cin, H, H, Cout, K, pad),
            "separate: bn_bwd_apply": lambda: ops.cl_bn_bwd_apply(y, gout, 0, scale, shift, coef, dy2, N, B, Cout,
                                                                  H, H),
            "separate: dgrad": lambda: ops.cl_conv_dgrad(dy, wk, dx, N, Cin, H, H, Cout, K, pad),
            "separate: wgrad": lambda: ops.cl_conv_wgrad(x, dy, wparts, N, Cin, H, H, Cout, K, pad),
            "pool": lambda: ops.cl_bn_relu_pool(y, scale, shift, pooled, 0, N, B, Cout, H, H),
            "pool + codes": lambda: ops.cl_bn_relu_pool_codes(y, scale, shift, pooled, codes, N, B, Cout, H, H)}
    us = {}
    for name, fn in runs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            fn()
        e.record()
        torch.cuda.synchronize()
        us[name] = s.elapsed_time(e) / 20 * 1e3
        print(f"{name}: {us[name]:.1f} us per launch", flush=True)
    print(f"separate: sum of the three {sum(v for k, v in us.items() if k.startswith('separate')):.1f} us", flush=True)


if __name__ == "__main__":
    main()
