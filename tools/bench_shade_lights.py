#!/usr/bin/env python3
"""Time one step of dirt_amd.deferred.shade_lights -- forward + backward -- against the framework-op statement and
against deferred.shade, on one GPU.

tools/bench_texture.py's method: one process; every leg is warmed up, captured into its own graph and replayed; the
rounds interleave the legs.  G-buffers: a disc of unit normals covering about 60 % of the frame over a -inf
background (a silhouette to dilate), frames of 512 x 512 (BASELINE config 4's) and 1024 x 1024; N = 1 (directional),
4 and 8 lights (alternating directional / point).  Legs per frame and N:
  fused_all    shade_lights with gradients to the three G-buffers and to every parameter (lights, camera, ambient
               colour, a tensor shininess): the forward, the backward's first kernel with its sums, the reducing kernel
  ops_all      `_shade_lights_ops`, the framework-op statement, with the same gradients
  fused_gbuf   shade_lights with gradients to the G-buffers only: no sums, no second launch (fused_all - fused_gbuf is
               the cost of the reduction)
  shade        N = 1 only: deferred.shade on the same inputs (gradients to the G-buffers; its parameters take none)
Prints one JSON line (and writes it to --out): per leg and round the milliseconds of one step.

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_shade_lights.py --profile --frame 512 --lights 4
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_texture import capture, time_graph  # noqa: E402
from dirt_amd import _lib, deferred  # noqa: E402

FRAMES = (512, 1024)
LIGHTS = (1, 4, 8)


def make_gbuffers(S, dev):
    """positions, colors, normals [S,S,3] float32: a disc of radius 0.44 S, -inf outside it"""
    rng = np.random.default_rng(S)
    yy, xx = np.mgrid[0:S, 0:S]
    covered = (yy - S / 2) ** 2 + (xx - S / 2) ** 2 <= (0.44 * S) ** 2
    n = rng.standard_normal((S, S, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    p = rng.uniform(-1.0, 1.0, (S, S, 3)).astype(np.float32)
    c = rng.uniform(0.2, 1.0, (S, S, 3)).astype(np.float32)
    p[~covered] = -np.inf
    n[~covered] = -np.inf
    return [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (p, c, n)], float(covered.mean())


def make_lights(N, dev):
    rng = np.random.default_rng(N)
    point = tuple(i % 2 == 1 for i in range(N))
    unit = rng.standard_normal((N, 3))
    unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
    vectors = unit * np.where(np.asarray(point)[:, None], 2.5, 1.0)  # point lights outside the positions' cube
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)  # noqa: E731
    return {"vectors": t(vectors), "diffuse": t(rng.uniform(0.1, 1.0, (N, 3))), "specular": t(rng.uniform(0.1, 1.0, (N, 3))),
            "camera": t([0.25, 1.75, 2.25]), "ambient": t([0.2, 0.2, 0.2]),
            "shininess": torch.tensor([6.0], device=dev)}, point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ops-iters", type=int, default=10, help="replays per timing of the (slow) framework-op legs")
    ap.add_argument("--frame", type=int, default=0, choices=(0,) + FRAMES, help="one frame size only")
    ap.add_argument("--lights", type=int, default=0, choices=(0,) + LIGHTS, help="one light count only")
    ap.add_argument("--profile", action="store_true", help="no timing: 10 eager fused_all steps per leg, for a profiler")
    ap.add_argument("--no-ops", action="store_true", help="the fused legs only (a variant library's run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"lib": os.path.basename(_lib.LIB_PATH), "iters": args.iters, "ops_iters": args.ops_iters, "legs": {}}
    legs = {}
    for S in (FRAMES if not args.frame else (args.frame,)):
        gbuf, coverage = make_gbuffers(S, dev)
        g = torch.randn((S, S, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        for N in (LIGHTS if not args.lights else (args.lights,)):
            ps, point = make_lights(N, dev)
            learn = {k: v.clone().requires_grad_(True) for k, v in ps.items()}
            order = ("vectors", "diffuse", "specular", "camera")

            def step(fn, p, k, wrt, gbuf=gbuf, point=point, g=g):
                pixels, _ = fn(*gbuf, *[p[n] for n in order], k, p["ambient"], point)
                return torch.autograd.grad(pixels, wrt, g)

            fns = {
                "fused_all": lambda s=step, p=learn, gb=gbuf: s(deferred.shade_lights, p, p["shininess"],
                                                                gb + list(p.values())),
                "ops_all": lambda s=step, p=learn, gb=gbuf: s(deferred._shade_lights_ops, p, p["shininess"],
                                                              gb + list(p.values())),
                "fused_gbuf": lambda s=step, p=ps, gb=gbuf: s(deferred.shade_lights, p, 6.0, gb),
            }
            if N == 1:
                def shade(p=ps, gbuf=gbuf, g=g):
                    pixels, _ = deferred.shade(*gbuf, p["ambient"], p["vectors"][0], p["diffuse"][0], p["specular"][0],
                                               p["camera"], 6.0, False)
                    return torch.autograd.grad(pixels, gbuf, g)
                fns["shade"] = shade
            if args.no_ops:
                del fns["ops_all"]
            key = "%dx%d N=%d" % (S, S, N)
            if args.profile:
                for _ in range(10):
                    fns["fused_all"]()
                torch.cuda.synchronize(dev)
                continue
            # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
            legs[key] = ({n: capture(f, dev) for n, f in fns.items()}, gbuf, ps, learn, g)
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
