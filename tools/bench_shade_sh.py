#!/usr/bin/env python3
"""Time one step of dirt_amd.deferred.shade_sh -- forward + backward -- against the framework-op statement and against
deferred.shade_lights, on one GPU.

tools/bench_shade_lights.py's method: one process; every leg is warmed up, captured into its own graph and replayed;
the rounds interleave the legs.  G-buffers: that tool's disc of unit normals covering about 60 % of the frame over a
-inf background (a silhouette to dilate), frames of 512 x 512 and 1024 x 1024; K = 4 and 9 coefficients, normals used
raw.  Legs per frame and K:
  fused_all     shade_sh with gradients to the colours, the normals and the coefficients: the forward, the backward's
                first kernel with its sums, the reducing kernel
  fused_gbuf    shade_sh with gradients to the two G-buffers only: no sums, no second launch (fused_all - fused_gbuf is
                the cost of the reduction)
  ops_all       `_shade_sh_ops`, the framework-op statement, in float32 with fused_all's gradients
  shade_lights  deferred.shade_lights with N = 1 directional light on the same G-buffers (and positions), gradients to
                the three G-buffers only: a familiar yardstick, the same for both K
Prints one JSON line (and writes it to --out): per leg and round the milliseconds of one step.

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_shade_sh.py --profile --frame 512 --coeffs 9
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_shade_lights import FRAMES, make_gbuffers, make_lights  # noqa: E402
from bench_texture import capture, time_graph  # noqa: E402
from dirt_amd import _lib, deferred  # noqa: E402

COEFFS = (4, 9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ops-iters", type=int, default=10, help="replays per timing of the (slow) framework-op legs")
    ap.add_argument("--frame", type=int, default=0, choices=(0,) + FRAMES, help="one frame size only")
    ap.add_argument("--coeffs", type=int, default=0, choices=(0,) + COEFFS, help="one coefficient count only")
    ap.add_argument("--profile", action="store_true", help="no timing: 10 eager fused_all steps per leg, for a profiler")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"lib": os.path.basename(_lib.LIB_PATH), "iters": args.iters, "ops_iters": args.ops_iters, "legs": {}}
    legs = {}
    for S in (FRAMES if not args.frame else (args.frame,)):
        gbuf, coverage = make_gbuffers(S, dev)
        positions, colors, normals = gbuf
        g = torch.randn((S, S, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        ps, point = make_lights(1, dev)
        for K in (COEFFS if not args.coeffs else (args.coeffs,)):
            coef = torch.from_numpy(np.random.default_rng(K).uniform(-1.0, 1.0, (K, 3)).astype(np.float32)).to(dev)
            learn = coef.clone().requires_grad_(True)

            def step(fn, c, wrt, colors=colors, normals=normals, g=g):
                pixels, _ = fn(colors, normals, c, None, False)
                return torch.autograd.grad(pixels, wrt, g)

            def lights(ps=ps, gbuf=gbuf, point=point, g=g):
                pixels, _ = deferred.shade_lights(*gbuf, ps["vectors"], ps["diffuse"], ps["specular"], ps["camera"],
                                                  6.0, ps["ambient"], point)
                return torch.autograd.grad(pixels, gbuf, g)

            all_, two = [colors, normals, learn], [colors, normals]
            fns = {
                "fused_all": lambda s=step, c=learn, w=all_: s(deferred.shade_sh, c, w),
                "fused_gbuf": lambda s=step, c=coef, w=two: s(deferred.shade_sh, c, w),
                "ops_all": lambda s=step, c=learn, w=all_: s(deferred._shade_sh_ops, c, w),
                "shade_lights": lights,
            }
            key = "%dx%d K=%d" % (S, S, K)
            if args.profile:
                for _ in range(10):
                    fns["fused_all"]()
                torch.cuda.synchronize(dev)
                continue
            # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
            legs[key] = ({n: capture(f, dev) for n, f in fns.items()}, gbuf, ps, coef, learn, g)
            result["legs"][key] = dict({n + "_ms": [] for n in fns}, coverage=round(coverage, 3))
    for _ in range(0 if args.profile else args.rounds):
        for key, (graphs, *_keep) in legs.items():
            for n, graph in graphs.items():
                iters = args.ops_iters if n.startswith("ops") else args.iters
                result["legs"][key][n + "_ms"].append(round(time_graph(graph, iters), 4))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
