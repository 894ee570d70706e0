#!/usr/bin/env python3
"""Time dirt_amd.deferred.sample_texture (forward + backward, gradients to the texture and the uv) against
torch.nn.functional.grid_sample (bilinear, border, align_corners=False: the same rule in clamp mode) on one GPU.

Legs: a 1024 x 1024 frame, C = 3, a seeded smooth uv warp with about 10 % unsampled (-inf) pixels, over textures of
2048^2 (minification), 1024^2 (about 1:1) and 64^2 (16x magnification).  One process; every leg is warmed up, captured
into its own graph and replayed; the rounds interleave yardstick and fused.  Prints one JSON line (and writes it to
--out): per leg and round the milliseconds of one forward + backward, and the bytes the backward adds atomically
(4 * C floats per sampled pixel on the direct path; the nonzero elements of each tile's patch on the LDS path, bounded
here by the tile's bounding box).

  DIRT_MI355X_LIB=build/variants/texture_direct.so python tools/bench_texture.py    # the direct-atomics-only build
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_texture.py --profile --leg 64   # kernel times
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dirt_amd import _lib, deferred  # noqa: E402

H = W = 1024
C = 3
LEGS = (2048, 1024, 64)
TILE = 16     # the backward's screen tile and
PATCH = 576   # LDS patch, in texels (kTexTile, kTexPatchTexels of dirt_amd/csrc/texture_kernels.h)


def make_uv(seed=0):
    """[H,W,2] float32: a smooth warp inside (0.03, 0.97), -inf outside a disc covering about 90 % of the frame"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, 4)
    u = 0.05 + 0.9 * x / W + 0.015 * np.sin(2 * np.pi * y / 300.0 + ph[0]) + 0.005 * np.sin(2 * np.pi * x / 70.0 + ph[1])
    v = 0.05 + 0.9 * y / H + 0.015 * np.sin(2 * np.pi * x / 260.0 + ph[2]) + 0.005 * np.sin(2 * np.pi * y / 90.0 + ph[3])
    uv = np.stack([u, v], -1).astype(np.float32)
    uv[(x - W / 2) ** 2 + (y - H / 2) ** 2 > (0.548 * W) ** 2] = -np.inf
    return uv


def atomic_bytes(uv, T):
    """(direct-path bytes, upper bound of the patch path's flush bytes, share of tiles whose box fits the patch)"""
    ok = np.isfinite(uv).all(-1)
    idx = []
    for k in (0, 1):
        x = np.clip(np.where(ok, uv[..., k], 0.0), 0.0, 1.0) * np.float32(T) - np.float32(0.5)
        j0 = np.clip(np.floor(x), -1, T).astype(np.int64)
        idx.append((np.clip(j0, 0, T - 1), np.clip(j0 + 1, 0, T - 1)))
    big = 1 << 30
    tiles = lambda a, fill, fn: fn(np.where(ok, a, fill).reshape(H // TILE, TILE, W // TILE, TILE), axis=(1, 3))  # noqa: E731
    bh = tiles(idx[1][1], -big, np.max) - tiles(idx[1][0], big, np.min) + 1
    bw = tiles(idx[0][1], -big, np.max) - tiles(idx[0][0], big, np.min) + 1
    any_ok = tiles(ok, False, np.max)
    per_tile_direct = tiles(ok.astype(np.int64), 0, np.sum) * 4 * C * 4
    fits = any_ok & (bh * bw <= PATCH)
    patch = np.where(fits, bh * bw * C * 4, np.where(any_ok, per_tile_direct, 0))
    return int(per_tile_direct.sum()), int(patch.sum()), float(fits.sum() / max(any_ok.sum(), 1))


def capture(step, dev):
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    graph.replay()
    torch.cuda.synchronize(dev)
    return graph


def time_graph(graph, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--leg", type=int, default=0, choices=(0,) + LEGS, help="one texture size only")
    ap.add_argument("--profile", action="store_true", help="no timing: 10 eager fused steps per leg, for a profiler")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    uv_np = make_uv()
    uv = torch.from_numpy(uv_np).to(dev).requires_grad_(True)
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.randn((H, W, C), device=dev, generator=gen)
    g_nchw = g.permute(2, 0, 1)[None].contiguous()
    result = {"lib": os.path.basename(_lib.LIB_PATH), "frame": [H, W], "channels": C, "iters": args.iters,
              "unsampled": float(1.0 - np.isfinite(uv_np).all(-1).mean()), "legs": {}}
    legs = {}
    for T in (LEGS if not args.leg else (args.leg,)):
        tex = torch.randn((T, T, C), device=dev, generator=gen).requires_grad_(True)
        tex_nchw = tex.detach().permute(2, 0, 1)[None].contiguous().requires_grad_(True)

        def fused(tex=tex):
            texels, _ = deferred.sample_texture(tex, uv)
            return torch.autograd.grad(texels, [tex, uv], g)

        def yardstick(tex_nchw=tex_nchw):
            out = Fn.grid_sample(tex_nchw, (2.0 * uv - 1.0)[None], mode="bilinear", padding_mode="border",
                                 align_corners=False)
            return torch.autograd.grad(out, [tex_nchw, uv], g_nchw)

        if args.profile:
            for _ in range(10):
                fused()
            torch.cuda.synchronize(dev)
            continue
        direct, patch, fits = atomic_bytes(uv_np, T)
        # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
        legs[T] = (capture(yardstick, dev), capture(fused, dev), tex, tex_nchw)
        result["legs"][str(T)] = {"yardstick_ms": [], "fused_ms": [], "atomic_bytes_direct": direct,
                                  "atomic_bytes_patch_bound": patch, "tiles_fitting_patch": fits}
    for _ in range(0 if args.profile else args.rounds):
        for T, (gy, gf, _tex, _tex_nchw) in legs.items():
            result["legs"][str(T)]["yardstick_ms"].append(round(time_graph(gy, args.iters), 4))
            result["legs"][str(T)]["fused_ms"].append(round(time_graph(gf, args.iters), 4))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
