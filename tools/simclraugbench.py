"""Time the view build of one SimCLR batch (AVMNISTSimCLRDataModule's four views: two image, two
spectrogram) with HIP events.
    python tools/simclraugbench.py [--batch 256] [--rounds 3] [--iters 50]

Per round, in microseconds:

  img x      the image chain (crop, rotation, affine, elastic p=0.3, blur p=0.3) through
             avd_augment_views_x, both views of the batch in one launch, records drawn beforehand;
  img x on   the same chain with the two new stages applied to every record (the worst batch);
  img seq    the chain's old stages only through avd_augment_views_seq -- what this launch cost
             before the two stages existed (the "without" baseline);
  img x old  those old stages through avd_augment_views_x (the template switch on, no new kind);
  aud        the spectrogram chain through the gather kernel, both views in one launch;
  records    the two parameter-draw launches (avd_augment_records_x, avd_augment_records);
  call       SimCLRMultiModalAugmentation.__call__ end to end (draws, id upload, both launches).

floor = the launch's HBM traffic (H*W source bytes + 4*H*W output bytes per view) at 6.3 TB/s, the
copy bandwidth measured on this part; the launches are far below the size where that binds, so
the floor is context, not a target."""
import argparse
import os
import sys

import numpy as np
import torch

HBM_BPS = 6.3e12


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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [tree, os.path.join(tree, "multimodal-ssl-avmnist_amd")]
    from avdino import augment as A
    from avdino import ops

    B, V, N = args.batch, 2, 4096
    rng = np.random.default_rng(0)
    dev = "cuda"
    ch = A.simclr_chains()
    img_old = [s for s in ch["image"] if s[0] not in A.X_KINDS]
    img_on = [(k, kw, 1.0) for k, kw, _p in ch["image"]]
    augs = {}
    for name, hw in (("image", 28), ("audio", 112)):
        src = torch.from_numpy(rng.integers(0, 256, (N, hw * hw), dtype=np.uint8)).to(dev)
        lut = torch.linspace(0, 1, 256, device=dev)
        augs[name] = A.ViewAugmenter(src, lut, hw, hw, seed=1)
    ia, aa = augs["image"], augs["audio"]
    idx = torch.from_numpy(rng.integers(0, N, B)).to(dev)
    out_i = torch.empty(V * B * 784, device=dev)
    out_a = torch.empty(V * B * 12544, device=dev)
    rec_x, _, ext_x = ia.records_dev(ch["image"], B, V)
    rec_on, _, ext_on = ia.records_dev(img_on, B, V)
    rec_o, _ = ia.records_dev(img_old, B, V)
    rec_a, _ = aa.records_dev(ch["audio"], B, V)
    kx, ko = A.chain_kinds(ch["image"]), A.chain_kinds(img_old)
    st_i, st_a = A.chain_stages(ch["image"], H=28, W=28), A.chain_stages(ch["audio"])

    def views_x(rec, ext, kinds):
        return lambda: ops.augment_views_x(ia.src, idx, ia.lut, rec, None, 4, 7, V, 28, 28, out_i, 1,
                                           kinds, ext)

    def records():
        ops.augment_records_x(st_i, B * V, 28, 28, 4, 11, rec_x, None, ext_x)
        ops.augment_records(st_a, B * V, 112, 112, 4, 12, rec_a, None)

    simclr = A.SimCLRMultiModalAugmentation().bind(ia, aa)
    idx_h = idx.cpu().numpy()
    legs = [
        ("img x", views_x(rec_x, ext_x, kx)),
        ("img x on", views_x(rec_on, ext_on, kx)),
        ("img seq", lambda: ops.augment_views(ia.src, idx, ia.lut, rec_o, None, 4, 7, V, 28, 28, out_i,
                                              1, ko)),
        ("img x old", views_x(rec_o, None, ko)),
        ("aud", lambda: ops.augment_views(aa.src, idx, aa.lut, rec_a, None, 4, 7, V, 112, 112, out_a, 1)),
        ("records", records),
        ("call", lambda: simclr(idx_h)),
    ]
    fl_i, fl_a = (V * B * 784 * 5 / HBM_BPS * 1e6, V * B * 12544 * 5 / HBM_BPS * 1e6)
    print(f"B={B}: floor image {fl_i:.2f} us, audio {fl_a:.2f} us (both views, {HBM_BPS / 1e12:.1f} TB/s); "
          f"elastic on {float((ext_x[:, 2] != 0).float().mean()):.2f}, "
          f"blur on {float((ext_x[:, 0] > 0).float().mean()):.2f} of the 'img x' records", flush=True)
    for r in range(args.rounds):
        cells = "  ".join(f"{name} {timeit(fn, args.iters):7.1f}" for name, fn in legs)
        print(f"round {r}: {cells}  (us)", flush=True)


if __name__ == "__main__":
    main()
