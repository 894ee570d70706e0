#!/usr/bin/env python3
"""Time one step of dirt_amd.deferred.sample_cubemap -- forward + backward -- against the framework-op statement and
against deferred.sample_texture, on one GPU.

tools/bench_shade_sh.py's method: one process; every leg is warmed up, captured into its own graph and replayed; the
rounds interleave the legs.  Frames of 512 x 512 and 1024 x 1024, C = 3, cube maps of S = 64 (magnified) and S = 1024
(about one texel a pixel).  Directions, a leaf tensor made before the timed step (r = i - 2 (n . i) n, i the unit view
ray), over the disc of tools/bench_shade_lights.py's G-buffers, -inf outside it:
  noise    that tool's G-buffers themselves: white-noise unit normals and positions, so neighbouring pixels look up
           unrelated faces, every screen tile straddles seams and the scatter goes straight to memory
  smooth   a unit sphere filling the disc, seen from (0, 0, 3): what a rendered object gives; at S = 64 most tiles lie
           on one face inside a few texels (the LDS patch), the rest on a seam
Legs per frame, S and direction set:
  fused_all       sample_cubemap with gradients to the cube map and the directions
  fused_dirs      sample_cubemap with the directions' gradient only: no scatter (fused_all - fused_dirs prices it)
  ops_all         `_sample_cubemap_ops`, the framework-op statement, in float32 with fused_all's gradients
  sample_texture  deferred.sample_texture of an S x S texture at the directions' own face coordinates (u, v), both
                  gradients: the same footprint without the face select, the divisions and the seams
Prints one JSON line (and writes it to --out): per leg and round the milliseconds of one step, and the share of the
screen tiles with a sampled pixel whose pixels lie on one face.

  make variant NAME=cube_nopatch DEFS=-DDIRT_CUBEMAP_PATCH=0    # the direct-atomics-only build, then
  DIRT_MI355X_LIB=build/variants/cube_nopatch.so python tools/bench_cubemap.py
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_cubemap.py --profile --frame 1024 --size 64
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_shade_lights import FRAMES, make_gbuffers, make_lights  # noqa: E402
from bench_texture import capture, time_graph  # noqa: E402
from dirt_amd import _lib, deferred  # noqa: E402

SIZES = (64, 1024)
SETS = ("noise", "smooth")
C = 3
TILE = 16  # the backward's screen tile (kTexTile of dirt_amd/csrc/texture_kernels.h)


def reflect(positions, normals, camera):
    ray = positions - camera
    i = ray / torch.linalg.norm(ray, dim=-1, keepdim=True)
    return i - 2.0 * (normals * i).sum(-1, keepdim=True) * normals


def make_directions(F, kind, dev):
    """[F,F,3] float32 reflection vectors over the disc, -inf outside it"""
    (positions, _, normals), _ = make_gbuffers(F, dev)
    positions, normals = positions.detach(), normals.detach()
    covered = torch.isfinite(normals).all(-1, keepdim=True)
    if kind == "noise":
        camera = make_lights(1, dev)[0]["camera"]
    else:
        yy, xx = torch.meshgrid(torch.arange(F, device=dev) + 0.5, torch.arange(F, device=dev) + 0.5, indexing="ij")
        nx, ny = (xx - F / 2) / (0.45 * F), -(yy - F / 2) / (0.45 * F)
        normals = torch.stack([nx, ny, torch.sqrt(torch.clamp(1.0 - nx * nx - ny * ny, min=0.0))], -1)
        positions, camera = normals, torch.tensor([0.0, 0.0, 3.0], device=dev)
    r = reflect(torch.where(covered, positions, 0.0), torch.where(covered, normals, 0.0), camera)
    return torch.where(covered, r, float("-inf")).contiguous()


def one_face_tiles(face, ok):
    """share of the 16 x 16 tiles with a sampled pixel whose sampled pixels lie on one face"""
    F = face.shape[0]
    t = lambda a: a.reshape(F // TILE, TILE, F // TILE, TILE).permute(0, 2, 1, 3).reshape(-1, TILE * TILE)  # noqa: E731
    lo = torch.where(t(ok), t(face), 9).min(-1).values
    hi = torch.where(t(ok), t(face), -1).max(-1).values
    some = t(ok).any(-1)
    return float(((lo == hi) & some).sum() / some.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ops-iters", type=int, default=10, help="replays per timing of the (slow) framework-op legs")
    ap.add_argument("--frame", type=int, default=0, choices=(0,) + FRAMES, help="one frame size only")
    ap.add_argument("--size", type=int, default=0, choices=(0,) + SIZES, help="one cube-map size only")
    ap.add_argument("--directions", default="", choices=("",) + SETS, help="one direction set only")
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all four)")
    ap.add_argument("--profile", action="store_true", help="no timing: 10 eager fused_all steps per leg, for a profiler")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"lib": os.path.basename(_lib.LIB_PATH), "iters": args.iters, "ops_iters": args.ops_iters, "channels": C,
              "legs": {}}
    legs = {}
    gen = torch.Generator(device=dev).manual_seed(1)
    for F in (FRAMES if not args.frame else (args.frame,)):
        g = torch.randn((F, F, C), device=dev, generator=gen)
        for kind in (SETS if not args.directions else (args.directions,)):
            d = make_directions(F, kind, dev).requires_grad_(True)
            with torch.no_grad():
                ok = torch.isfinite(d).all(-1)
                face, u, v = deferred._cube_coordinates(d, ok)
                uv = torch.where(ok[..., None], torch.stack([u, v], -1), float("-inf")).contiguous()
            uv.requires_grad_(True)
            for S in (SIZES if not args.size else (args.size,)):
                cube = torch.randn((6, S, S, C), device=dev, generator=gen)
                learn = cube.clone().requires_grad_(True)
                tex = cube[0].clone().requires_grad_(True)

                def step(fn, c, wrt, d=d, g=g):
                    texels, _ = fn(c, d)
                    return torch.autograd.grad(texels, wrt, g)

                fns = {
                    "fused_all": lambda s=step, c=learn, d=d: s(deferred.sample_cubemap, c, [c, d]),
                    "fused_dirs": lambda s=step, c=cube, d=d: s(deferred.sample_cubemap, c, [d]),
                    "ops_all": lambda s=step, c=learn, d=d: s(deferred._sample_cubemap_ops, c, [c, d]),
                    "sample_texture": lambda s=step, t=tex, uv=uv: s(deferred.sample_texture, t, [t, uv], uv),
                }
                if args.legs:
                    fns = {n: fns[n] for n in args.legs.split(",")}
                key = "%dx%d S=%d %s" % (F, F, S, kind)
                if args.profile:
                    for _ in range(10):
                        fns["fused_all"]()
                    torch.cuda.synchronize(dev)
                    continue
                # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
                legs[key] = ({n: capture(f, dev) for n, f in fns.items()}, d, uv, cube, learn, tex, g)
                result["legs"][key] = dict({n + "_ms": [] for n in fns}, sampled=round(float(ok.float().mean()), 3),
                                           one_face_tiles=round(one_face_tiles(face, ok), 3))
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
