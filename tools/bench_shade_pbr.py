#!/usr/bin/env python3
"""Time one step of dirt_amd.deferred.shade_pbr -- forward + backward -- against the framework-op statement and against
deferred.shade_lights at the same light count, on one GPU.

tools/bench_shade_lights.py's method and G-buffers: one process; every leg is warmed up, captured into its own graph
and replayed; the rounds interleave the legs.  A disc of unit normals covering about 60 % of the frame over a -inf
background, frames of 512 x 512 and 1024 x 1024; N = 1 (directional), 4 and 8 lights (alternating directional /
point); roughness in [0.2, 1], metallic in [0, 1], a visibility in [0, 1] per pixel and light.  Legs per frame and N:
  fused_all     shade_pbr with every gradient: the three G-buffers, the material, the visibility and every parameter
                (lights, camera, ambient colour): the forward, the backward's first kernel with its sums, the reducing
                kernel
  fused_gbuf    shade_pbr with gradients to the three G-buffers and the material only: no sums, no second launch
  ops_all       `_shade_pbr_ops`, the framework-op statement, with fused_all's gradients
  shade_lights  deferred.shade_lights under the same lights with every one of its gradients: the neighbouring yardstick
Prints one JSON line (and writes it to --out): per leg and round the milliseconds of one step.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_shade_lights import make_gbuffers, make_lights  # noqa: E402
from bench_texture import capture, time_graph  # noqa: E402
from dirt_amd import _lib, deferred  # noqa: E402

FRAMES = (512, 1024)
LIGHTS = (1, 4, 8)


def make_material(S, N, dev):
    """material [S,S,2] (roughness in [0.2, 1], metallic in [0, 1]) and visibility [S,S,N] in [0, 1]"""
    rng = np.random.default_rng([S, N])
    mat = np.stack([rng.uniform(0.2, 1.0, (S, S)), rng.uniform(0.0, 1.0, (S, S))], -1).astype(np.float32)
    vis = rng.uniform(0.0, 1.0, (S, S, N)).astype(np.float32)
    return [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (mat, vis)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ops-iters", type=int, default=10, help="replays per timing of the (slow) framework-op legs")
    ap.add_argument("--frame", type=int, default=0, choices=(0,) + FRAMES, help="one frame size only")
    ap.add_argument("--lights", type=int, default=0, choices=(0,) + LIGHTS, help="one light count only")
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
            mat, vis = make_material(S, N, dev)
            pbr_params = ("vectors", "diffuse", "camera", "ambient")

            def pbr(fn, p, wrt, gbuf=gbuf, mat=mat, vis=vis, point=point, g=g):
                pixels, _ = fn(*gbuf, mat, p["vectors"], p["diffuse"], p["camera"], p["ambient"], point, vis)
                return torch.autograd.grad(pixels, wrt, g)

            def lights(p=learn, gbuf=gbuf, point=point, g=g):
                pixels, _ = deferred.shade_lights(*gbuf, p["vectors"], p["diffuse"], p["specular"], p["camera"],
                                                  p["shininess"], p["ambient"], point)
                return torch.autograd.grad(pixels, gbuf + list(p.values()), g)

            every = gbuf + [mat, vis] + [learn[k] for k in pbr_params]
            fns = {
                "fused_all": lambda f=pbr, p=learn, w=every: f(deferred.shade_pbr, p, w),
                "fused_gbuf": lambda f=pbr, p=ps, w=gbuf + [mat]: f(deferred.shade_pbr, p, w),
                "ops_all": lambda f=pbr, p=learn, w=every: f(deferred._shade_pbr_ops, p, w),
                "shade_lights": lights,
            }
            if args.no_ops:
                del fns["ops_all"]
            key = "%dx%d N=%d" % (S, S, N)
            # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
            legs[key] = ({n: capture(f, dev) for n, f in fns.items()}, gbuf, ps, learn, mat, vis, g)
            result["legs"][key] = dict({n + "_ms": [] for n in fns}, coverage=round(coverage, 3))
    for _ in range(args.rounds):
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
