#!/usr/bin/env python3
"""Time one step of mipmapped texturing -- dirt_amd.deferred.build_mipmaps + sample_texture_mip, forward + backward,
gradients to the texture and the uv -- against a framework-op yardstick, on one GPU.

tools/bench_texture.py's method: its 1024 x 1024 frame, C = 3, its seeded smooth uv warp with about 10 % unsampled
(-inf) pixels, its textures of 2048^2 (2x minification), 1024^2 (about 1:1) and 64^2 (16x magnification), clamp mode.
One process; every leg is warmed up, captured into its own graph and replayed; the rounds interleave the legs.  Legs:
  fused      build_mipmaps + sample_texture_mip of the library this process loaded (DIRT_MI355X_LIB picks a variant)
  yardstick  an avg_pool2d chain, grid_sample(bilinear, border, align_corners=False) at every level, a gather of the
             two levels of each pixel's lod and a lerp; the lod is the fused forward's, handed over as a constant
  bilinear   for information: the existing sample_texture on the same inputs (no chain)
Prints one JSON line (and writes it to --out): per leg and round the milliseconds of one step.

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_texture_mip.py --profile --leg 2048   # kernel times
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_texture import C, H, LEGS, W, capture, make_uv, time_graph  # noqa: E402
from dirt_amd import _lib, deferred  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--yardstick-iters", type=int, default=5, help="replays per timing of the (slow) yardstick")
    ap.add_argument("--leg", type=int, default=0, choices=(0,) + LEGS, help="one texture size only")
    ap.add_argument("--profile", action="store_true", help="no timing: 10 eager fused steps per leg, for a profiler")
    ap.add_argument("--no-yardstick", action="store_true", help="fused and bilinear only (a variant library's run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    uv = torch.from_numpy(make_uv()).to(dev).requires_grad_(True)
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.randn((H, W, C), device=dev, generator=gen)
    result = {"lib": os.path.basename(_lib.LIB_PATH), "frame": [H, W], "channels": C, "iters": args.iters,
              "yardstick_iters": args.yardstick_iters, "legs": {}}
    legs = {}
    for T in (LEGS if not args.leg else (args.leg,)):
        tex = torch.randn((T, T, C), device=dev, generator=gen).requires_grad_(True)
        with torch.no_grad():
            lod = deferred._sample_texture_mip(tex, uv)[2]
        L = len(deferred._mip_dims(T, T))
        sampled = lod[torch.isfinite(uv).all(-1)]
        k0 = lod.floor().long()
        k1 = torch.clamp(k0 + 1, max=L - 1)
        f = (lod - k0)[..., None]

        def fused(tex=tex):
            texels, _ = deferred.sample_texture_mip(tex, uv)
            return torch.autograd.grad(texels, [tex, uv], g)

        def bilinear(tex=tex):
            texels, _ = deferred.sample_texture(tex, uv)
            return torch.autograd.grad(texels, [tex, uv], g)

        def yardstick(tex=tex, k0=k0, k1=k1, f=f, L=L):
            levels = [tex.permute(2, 0, 1)[None]]
            for _ in range(1, L):
                levels.append(Fn.avg_pool2d(levels[-1], 2))
            grid = (2.0 * uv - 1.0)[None]
            per_level = torch.stack([Fn.grid_sample(t, grid, mode="bilinear", padding_mode="border",
                                                    align_corners=False)[0].permute(1, 2, 0) for t in levels])
            pick = lambda k: torch.gather(per_level, 0, k[None, ..., None].expand((1, H, W, C)))[0]  # noqa: E731
            out = pick(k0) * (1.0 - f) + pick(k1) * f
            out = torch.where(torch.isfinite(uv).all(-1, keepdim=True), out, 0.0)
            return torch.autograd.grad(out, [tex, uv], g)

        if args.profile:
            for _ in range(10):
                fused()
            torch.cuda.synchronize(dev)
            continue
        names = ["fused", "bilinear"] + ([] if args.no_yardstick else ["yardstick"])
        fns = {"fused": fused, "bilinear": bilinear, "yardstick": yardstick}
        # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
        legs[T] = ({n: capture(fns[n], dev) for n in names}, tex, k0, k1, f)
        result["legs"][str(T)] = dict({n + "_ms": [] for n in names}, levels=L,
                                      lod=[round(float(x), 3) for x in (sampled.min(), sampled.median(),
                                                                        sampled.max())])
    for _ in range(0 if args.profile else args.rounds):
        for T, (graphs, *_keep) in legs.items():
            for n, graph in graphs.items():
                iters = args.yardstick_iters if n == "yardstick" else args.iters
                result["legs"][str(T)][n + "_ms"].append(round(time_graph(graph, iters), 4))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
