#!/usr/bin/env python3
"""Time dirt_amd.deferred.sample_shadow (forward + backward, gradients to the depth map, the positions and the light
matrix) on one GPU against
  ops:      `_sample_shadow_ops`, the framework-op statement, on the same inputs;
  texture:  deferred.sample_texture with C = 1 on the same (u, v) footprint over the same map, gradients to the texture
            and the uv -- the sibling that bounds what the lookup alone can cost;
  no_matrix: sample_shadow without the light matrix's gradient (no partial sums, no second launch): the difference to
            the full step is the share of the matrix sums.

Legs: two frames of 512^2 or 1024^2 world positions (a rippled receiver under an orthographic light, about 10 %
background) over a 256^2 or 2048^2 depth map (16x to 1/2x magnification), softness 0 or > 0, the matrix shared or one
per frame.  One process; every leg is warmed up, captured into its own graph and replayed; the rounds interleave the
four variants.  Prints one JSON line (and writes it to --out): per leg the median and the extremes over the rounds
of the milliseconds of one forward + backward.

  DIRT_MI355X_LIB=build/variants/shadow_direct.so python tools/bench_shadow.py   # make variant NAME=shadow_direct
                                                                                  #   DEFS=-DDIRT_TEXTURE_PATCH=0
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dirt_amd import _lib, deferred  # noqa: E402

B = 2
FRAMES = (512, 1024)
MAPS = (256, 2048)
BIAS = 0.01


def light_matrix():
    """an orthographic light looking down -z over the box |x|, |y| <= 1, clip z = 1 - z"""
    return np.array([[1., 0., 0., 0.], [0., 1., 0., 0.], [0., 0., -1., 0.], [0., 0., 1., 1.]], np.float32)


def make_positions(N, seed=0):
    """[B,N,N,3] float32: a smooth warp of the frame onto (-0.94, 0.94)^2 with a rippled height, -inf outside a disc
    covering about 90 % of the frame"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(N) + 0.5, np.arange(N) + 0.5, indexing="ij")
    frames = []
    for _ in range(B):
        ph = rng.uniform(0, 2 * np.pi, 6)
        px = -0.9 + 1.8 * x / N + 0.03 * np.sin(2 * np.pi * y / (0.3 * N) + ph[0]) + 0.01 * np.sin(2 * np.pi * x / (0.07 * N) + ph[1])
        py = -0.9 + 1.8 * y / N + 0.03 * np.sin(2 * np.pi * x / (0.26 * N) + ph[2]) + 0.01 * np.sin(2 * np.pi * y / (0.09 * N) + ph[3])
        pz = 0.2 * np.sin(3.0 * px + ph[4]) * np.cos(2.0 * py + ph[5])
        p = np.stack([px, py, pz], -1).astype(np.float32)
        p[(x - N / 2) ** 2 + (y - N / 2) ** 2 > (0.548 * N) ** 2] = -np.inf
        frames.append(p)
    return np.stack(frames)


def make_depth(S, seed=1):
    """[S,S,1] float32 clip z: a smooth occluder field that crosses the receiver's (lit, shadowed and ramp pixels),
    +inf (nothing drawn) on about a tenth of the map"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, 2)
    d = 1.0 + 0.25 * np.sin(2 * np.pi * i / S * 3 + ph[0]) * np.cos(2 * np.pi * j / S * 2 + ph[1])
    d = d.astype(np.float32)
    d[(np.sin(2 * np.pi * i / S * 5) * np.sin(2 * np.pi * j / S * 5)) > 0.8] = np.inf
    return d[..., None]


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frame", type=int, default=0, choices=(0,) + FRAMES, help="one frame size only")
    ap.add_argument("--no-ops", action="store_true", help="leave the framework-op statement out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    M_np = light_matrix()
    result = {"lib": os.path.basename(_lib.LIB_PATH), "frames": B, "iters": args.iters, "rounds": args.rounds,
              "bias": BIAS, "legs": {}}
    legs = {}
    for N in (FRAMES if not args.frame else (args.frame,)):
        pos_np = make_positions(N)
        pos = torch.from_numpy(pos_np).to(dev).requires_grad_(True)
        g = torch.randn((B, N, N, 1), device=dev, generator=gen)
        # the footprint for the texture sibling: the rule's (u, v) of the sampled pixels, -inf elsewhere
        with torch.no_grad():
            clip = torch.cat([pos, torch.ones_like(pos[..., :1])], -1) @ torch.from_numpy(M_np).to(dev)
            uv = torch.stack([clip[..., 0] * 0.5 + 0.5, 0.5 - clip[..., 1] * 0.5], -1)
            uv = torch.where(torch.isfinite(pos).all(-1, keepdim=True), uv, float("-inf")).contiguous()
        uv.requires_grad_(True)
        for S in MAPS:
            depth_np = make_depth(S)
            depth = torch.from_numpy(depth_np).to(dev).requires_grad_(True)
            tex = torch.from_numpy(np.where(np.isfinite(depth_np), depth_np, 2.0).astype(np.float32)).to(dev)
            tex.requires_grad_(True)
            for softness in (0.0, 0.05):
                for per_frame in (False, True):
                    M = torch.from_numpy(np.stack([M_np] * B) if per_frame else M_np).to(dev).requires_grad_(True)
                    M_const = M.detach().clone()

                    def fused(depth=depth, M=M, softness=softness):
                        vis, _ = deferred.sample_shadow(depth, pos, M, BIAS, softness)
                        return torch.autograd.grad(vis, [depth, pos, M], g)

                    def no_matrix(depth=depth, M=M_const, softness=softness):
                        vis, _ = deferred.sample_shadow(depth, pos, M, BIAS, softness)
                        return torch.autograd.grad(vis, [depth, pos], g)

                    def ops(depth=depth, M=M, softness=softness):
                        vis, _ = deferred._sample_shadow_ops(depth, pos, M, BIAS, softness)
                        return torch.autograd.grad(vis, [depth, pos, M] if softness > 0 else [pos, M], g)

                    def texture(tex=tex):
                        texels, _ = deferred.sample_texture(tex, uv)
                        return torch.autograd.grad(texels, [tex, uv], g)

                    name = "%d/%d/%s/%s" % (N, S, "soft" if softness > 0 else "hard", "perframe" if per_frame else "shared")
                    variants = {"fused": fused, "no_matrix": no_matrix, "texture": texture}
                    if not args.no_ops:
                        variants["ops"] = ops
                    # (the graphs replay on the captured addresses: their inputs stay alive as long as they do)
                    legs[name] = ({k: capture(fn, dev) for k, fn in variants.items()}, (depth, tex, M, M_const, pos, uv, g))
                    result["legs"][name] = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, (graphs, _keep) in legs.items():
            for k, graph in graphs.items():
                result["legs"][name][k].append(time_graph(graph, args.iters))
    for name, times in result["legs"].items():
        med = {k: statistics.median(v) for k, v in times.items()}
        result["legs"][name] = {k: {"median_ms": round(med[k], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                                for k, v in times.items()}
        result["legs"][name]["matrix_sums_share"] = round(1.0 - med["no_matrix"] / med["fused"], 4)
        if "ops" in med:
            result["legs"][name]["ops_over_fused"] = round(med["ops"] / med["fused"], 2)
        result["legs"][name]["fused_over_texture"] = round(med["fused"] / med["texture"], 3)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
