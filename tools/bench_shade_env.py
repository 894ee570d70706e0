#!/usr/bin/env python3
"""Time one step of dirt_amd.deferred.shade_env, of deferred.reflect_view and of the image-based-lighting chain they
close -- forward + backward -- against the framework-op statements and against deferred.shade_pbr at N = 1, on one
GPU.

tools/bench_shade_pbr.py's method and G-buffers: one process; every leg is warmed up, captured into its own graph and
replayed; the rounds interleave the legs.  A disc of unit normals covering about 60 % of the frame over a -inf
background, frames of 512 x 512 and 1024 x 1024; K = 9 coefficients; roughness in [0.2, 1], metallic in [0, 1], a
radiance in [0, 2] and an occlusion in [0.2, 1] per pixel.  Legs per frame:
  env_fused_all      shade_env with every gradient: the three G-buffers, the material, the radiance, the occlusion, the
                     coefficients and the camera: the forward, the backward's first kernel with its sums, the reducing
                     kernel
  env_fused_gbuf     shade_env with gradients to the three G-buffers, the material and the radiance only: no sums, no
                     second launch
  env_ops_all        `_shade_env_ops`, the framework-op statement, with env_fused_all's gradients
  reflect_fused_all  reflect_view with gradients to positions, normals and the camera
  reflect_ops_all    `_reflect_view_ops` with the same gradients
  shade_pbr          deferred.shade_pbr under one directional light with every one of its gradients: the yardstick
and per cube-map size S = 64 and S = 1024 (the chain built before the timed step, `packed` the leaf):
  chain_fused S=..   reflect_view -> sample_cubemap_mip at lod = roughness (levels - 1) -> shade_env, with gradients to
                     the G-buffers, the material, the occlusion, the coefficients, the camera and the cube chain
  chain_ops S=..     the same chain with every op on its framework-op statement; timed eagerly between two events
                     (`_sample_cubemap_mip_ops` asks the device which levels are in use, which no capture allows)
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
from bench_cubemap_mip import Eager  # noqa: E402
from bench_shade_lights import make_gbuffers, make_lights  # noqa: E402
from bench_shade_pbr import make_material  # noqa: E402
from bench_texture import capture, time_graph  # noqa: E402
from dirt_amd import _lib, deferred  # noqa: E402

FRAMES = (512, 1024)
CUBES = (64, 1024)
K = 9


def make_env(S, dev):
    """radiance [S,S,3] in [0, 2], occlusion [S,S,1] in [0.2, 1], coefficients [K,3], camera [3]"""
    rng = np.random.default_rng([S, K])
    coef = rng.uniform(-1.0, 1.0, (K, 3))
    coef[0] = rng.uniform(0.5, 1.5, 3)
    arrays = (rng.uniform(0.0, 2.0, (S, S, 3)), rng.uniform(0.2, 1.0, (S, S, 1)), coef, [0.25, 1.75, 2.25])
    return [torch.from_numpy(np.asarray(a, np.float32)).to(dev).requires_grad_(True) for a in arrays]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ops-iters", type=int, default=10, help="replays per timing of the (slow) framework-op legs")
    ap.add_argument("--chain-ops-iters", type=int, default=1, help="steps per timing of the eager chain_ops legs")
    ap.add_argument("--frame", type=int, default=0, choices=(0,) + FRAMES, help="one frame size only")
    ap.add_argument("--no-ops", action="store_true", help="the fused legs only (a variant library's run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"lib": os.path.basename(_lib.LIB_PATH), "iters": args.iters, "ops_iters": args.ops_iters,
              "chain_ops_iters": args.chain_ops_iters, "coefficients": K, "legs": {}}
    legs = {}
    gen = torch.Generator(device=dev).manual_seed(1)
    chains = {}
    for S in CUBES:
        with torch.no_grad():
            built = deferred.build_cubemap_mipmaps(torch.rand((6, S, S, 3), device=dev, generator=gen) + 0.1)
        packed = built.packed.clone().requires_grad_(True)
        chains[S] = (deferred.CubeMipmaps(packed, S), packed)
    for F in (FRAMES if not args.frame else (args.frame,)):
        gbuf, coverage = make_gbuffers(F, dev)
        pos, col, nrm = gbuf
        g = torch.randn((F, F, 3), device=dev, generator=gen)
        mat, _ = make_material(F, 1, dev)
        rad, occ, coef, cam = make_env(F, dev)
        lights, point = make_lights(1, dev)
        lights = {k: v.clone().requires_grad_(True) for k, v in lights.items()}
        vis = torch.rand((F, F, 1), device=dev, generator=gen).requires_grad_(True)

        def env(fn, wrt, g=g, gbuf=gbuf, mat=mat, rad=rad, occ=occ, coef=coef, cam=cam):
            pixels, _ = fn(*gbuf, mat, coef, rad, cam, occ)
            return torch.autograd.grad(pixels, wrt, g)

        def reflect(fn, g=g, pos=pos, nrm=nrm, cam=cam):
            directions, _ = fn(pos, nrm, cam)
            return torch.autograd.grad(directions, [pos, nrm, cam], g)

        def pbr(g=g, gbuf=gbuf, mat=mat, vis=vis, p=lights, point=point):
            params = [p[k] for k in ("vectors", "diffuse", "camera", "ambient")]
            pixels, _ = deferred.shade_pbr(*gbuf, mat, *params, point, vis)
            return torch.autograd.grad(pixels, gbuf + [mat, vis] + params, g)

        def chain(fused, S, g=g, gbuf=gbuf, mat=mat, occ=occ, coef=coef, cam=cam):
            cube, packed = chains[S]
            reflect_fn, sample_fn, env_fn = (
                (deferred.reflect_view, deferred.sample_cubemap_mip, deferred.shade_env) if fused else
                (deferred._reflect_view_ops, deferred._sample_cubemap_mip_ops, deferred._shade_env_ops))
            directions = reflect_fn(gbuf[0], gbuf[2], cam)[0]
            radiance = sample_fn(cube, directions, None, mat[..., 0] * (len(cube) - 1))[0]
            pixels = env_fn(*gbuf, mat, coef, radiance, cam, occ)[0]
            return torch.autograd.grad(pixels, gbuf + [mat, occ, coef, cam, packed], g)

        every = gbuf + [mat, rad, occ, coef, cam]
        fns = {
            "env_fused_all": lambda w=every: env(deferred.shade_env, w),
            "env_fused_gbuf": lambda w=gbuf + [mat, rad]: env(deferred.shade_env, w),
            "env_ops_all": lambda w=every: env(deferred._shade_env_ops, w),
            "reflect_fused_all": lambda: reflect(deferred.reflect_view),
            "reflect_ops_all": lambda: reflect(deferred._reflect_view_ops),
            "shade_pbr": pbr,
        }
        for S in CUBES:
            fns["chain_fused S=%d" % S] = lambda S=S: chain(True, S)
            fns["chain_ops S=%d" % S] = lambda S=S: chain(False, S)
        if args.no_ops:
            fns = {n: f for n, f in fns.items() if "_ops" not in n}
        key = "%dx%d K=%d" % (F, F, K)
        # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
        timed = {n: Eager(f, dev) if n.startswith("chain_ops") else capture(f, dev) for n, f in fns.items()}
        legs[key] = (timed, gbuf, g, mat, rad, occ, coef, cam, lights, vis)
        result["legs"][key] = dict({n + "_ms": [] for n in fns}, coverage=round(coverage, 3))
    for _ in range(args.rounds):
        for key, (graphs, *_keep) in legs.items():
            for n, graph in graphs.items():
                iters = args.chain_ops_iters if n.startswith("chain_ops") else \
                    args.ops_iters if "_ops" in n else args.iters
                result["legs"][key][n + "_ms"].append(round(time_graph(graph, iters), 4))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
