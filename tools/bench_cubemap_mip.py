#!/usr/bin/env python3
"""Time one step of dirt_amd.deferred.sample_cubemap_mip -- forward + backward -- against the framework-op statement
and against deferred.sample_cubemap, on one GPU.

tools/bench_cubemap.py's method and inputs: one process; every leg is warmed up, captured into its own graph and
replayed; the rounds interleave the legs.  Frames of 1024 x 1024 (512 x 512 with --frame), C = 3, cube maps of S = 64
and S = 1024 whose chain is built before the timed step (`packed` is the leaf), the reflection vectors of that tool
(`noise`: every tile straddles seams; `smooth`: a sphere, what a rendered object gives).  Level of detail:
  zero   an explicit lod of 0 everywhere: sample_cubemap's work, plus the seams and the lod's plumbing
  ramp   an explicit lod growing from 0 to levels - 1 across the frame's width: a roughness ramp, every level in use
  auto   lod=None: taken from the directions
Legs per S, direction set and lod:
  fused_all       sample_cubemap_mip with gradients to the chain, the directions and (zero, ramp) the lod
  fused_gathers   the directions' and the lod's gradients only: no scatter (fused_all - fused_gathers prices it)
  ops_all         `_sample_cubemap_mip_ops`, the framework-op statement, in float32 with fused_all's gradients; timed
                  eagerly between two events (it asks the device which levels are in use, which no capture allows)
  sample_cubemap  (zero only) deferred.sample_cubemap of level 0 with its two gradients
Prints one JSON line (and writes it to --out): per leg and round the milliseconds of one step.

  make variant NAME=cubemip_nopatch DEFS=-DDIRT_CUBEMAP_MIP_PATCH=0    # the direct-atomics-only build, then
  DIRT_MI355X_LIB=build/variants/cubemip_nopatch.so python tools/bench_cubemap_mip.py --legs fused_all
  python tools/bench_cubemap_mip.py --legs ops_all --rounds 3     # seconds a step: a process of its own
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_cubemap_mip.py --profile --size 64 --lod ramp
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_cubemap import SETS, SIZES, C, make_directions  # noqa: E402
from bench_shade_lights import FRAMES  # noqa: E402
from bench_texture import capture, time_graph  # noqa: E402
from dirt_amd import _lib, deferred  # noqa: E402

LODS = ("zero", "ramp", "auto")


class Eager:
    """a step that cannot be captured, with a graph's replay()"""

    def __init__(self, step, dev):
        self.replay = step
        step()
        torch.cuda.synchronize(dev)


def make_lod(kind, F, levels, dev):
    if kind == "auto":
        return None
    if kind == "zero":
        return torch.zeros((F, F), device=dev).requires_grad_(True)
    ramp = torch.linspace(0.0, float(levels - 1), F, device=dev)
    return ramp[None, :].expand(F, F).contiguous().requires_grad_(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ops-iters", type=int, default=1, help="steps per timing of the (slow) framework-op legs")
    ap.add_argument("--frame", type=int, default=1024, choices=FRAMES)
    ap.add_argument("--size", type=int, default=0, choices=(0,) + SIZES, help="one cube-map size only")
    ap.add_argument("--directions", default="", choices=("",) + SETS, help="one direction set only")
    ap.add_argument("--lod", default="", choices=("",) + LODS, help="one lod mode only")
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
    ap.add_argument("--profile", action="store_true", help="no timing: 10 eager fused_all steps per leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    F = args.frame
    result = {"lib": os.path.basename(_lib.LIB_PATH), "iters": args.iters, "ops_iters": args.ops_iters, "channels": C,
              "frame": F, "legs": {}}
    legs = {}
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.randn((F, F, C), device=dev, generator=gen)
    for kind in (SETS if not args.directions else (args.directions,)):
        d = make_directions(F, kind, dev).requires_grad_(True)
        for S in (SIZES if not args.size else (args.size,)):
            cube = torch.randn((6, S, S, C), device=dev, generator=gen)
            learn = cube.clone().requires_grad_(True)
            with torch.no_grad():
                built = deferred.build_cubemap_mipmaps(cube)
            packed = built.packed.clone().requires_grad_(True)
            chain = deferred.CubeMipmaps(packed, S)
            fixed = deferred.CubeMipmaps(built.packed, S)
            for mode in (LODS if not args.lod else (args.lod,)):
                lod = make_lod(mode, F, len(chain), dev)
                gathers = [d] + ([lod] if lod is not None else [])

                def step(fn, c, wrt, lod=lod, d=d, g=g):
                    texels = fn(c, d, None, lod)[0]
                    return torch.autograd.grad(texels, wrt, g)

                fns = {
                    "fused_all": lambda s=step, c=chain, w=[packed] + gathers: s(deferred.sample_cubemap_mip, c, w),
                    "fused_gathers": lambda s=step, c=fixed, w=gathers: s(deferred.sample_cubemap_mip, c, w),
                    "ops_all": lambda s=step, c=chain, w=[packed] + gathers: s(deferred._sample_cubemap_mip_ops, c, w),
                }
                if mode == "zero":
                    fns["sample_cubemap"] = lambda c=learn, d=d, g=g: torch.autograd.grad(
                        deferred.sample_cubemap(c, d)[0], [c, d], g)
                if args.legs:
                    fns = {n: fns[n] for n in args.legs.split(",") if n in fns}
                key = "%dx%d S=%d %s lod=%s" % (F, F, S, kind, mode)
                if args.profile:
                    for _ in range(10):
                        fns["fused_all"]()
                    torch.cuda.synchronize(dev)
                    continue
                # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
                timed = {n: Eager(f, dev) if n.startswith("ops") else capture(f, dev) for n, f in fns.items()}
                legs[key] = (timed, d, cube, learn, packed, built, lod, g)
                result["legs"][key] = dict({n + "_ms": [] for n in fns}, levels=len(chain))
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
