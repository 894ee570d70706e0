"""GPU pin of the rasteriser at full frame size (tests/large_frame_cases.py: 4096x4096, 4097x4097, 8192x2049,
8192x8192): the regimes that only large frames reach -- the 128-px coarse tile (cshift = 7) with its 7-bit relative
bounding boxes, a full coarse histogram, 2^18 tiles in grid.x, both pixel coordinates large at once.

Forward, every case: the whole frame bit-exact against the oracle on the device (pixels, g-buffer word, depth,
barycentrics, face ids, plain and G-buffer rasters), and every window of the HIP outputs against the exact statement
(tests/forward_exact.py) directly -- no oracle value takes part in that comparison.  The other forward paths (an
explicit bin_capacity that overflows some slabs of 128-px tiles and not others, the resolve-only second render of
shared geometry, the deep-cull raster forced, at most 32 faces -- which a large frame does NOT route to the fused
small-scene raster: asserted) on one 8192x8192 and one 4097x4097 case.  oceanic_horizon and hill once each on
8192x2049 against the oracle alone: there is no independent statement of the procedural programs.

Backward, every window of every case, cotangents supported on the window, through the public path: the
per-element bound of tests/backward_cases.py against the windowed float64 statement; elements without terms --
every vertex that does not reach the window -- exactly zero, so a stray contribution from any of the 2^18 tiles
fails; grad_background checked on the device over the whole frame.  One dense-cotangent backward per frame size
against the oracle under the strict pair of test_gpu_parity.assert_close_grad, the only affordable contract for
all tiles at once, on the scene without its frame-sized faces (the test says why).  65537 frames of 4x4 pixels: the
batch in grid.y past 16 bits.

Every test prints its figures (run with -s); DESIGN.md 5 collects them.
"""
import ctypes

import numpy as np
import pytest
import torch

import backward_cases as bc
import large_frame_cases as lf
import scenes
from oracle import oracle
from test_gpu_parity import STRICT, assert_close_grad

pytestmark = pytest.mark.gpu

PATH_CASES = ["8192x8192_c1", "4097x4097_c5"]
DENSE_CASES = ["4096x4096_c3", "4097x4097_c7", "8192x2049_c3", "8192x8192_c1"]  # one per frame size
_dev_cache = {}


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device(name):
    """The case's inputs and the oracle's pixels and g-buffer on the device (one case at a time)."""
    if name not in _dev_cache:
        _dev_cache.clear()
        torch.cuda.empty_cache()
        b = lf.bulk(name)
        _dev_cache[name] = tuple(_gpu(a) for a in b.inputs) + (_gpu(b.px), _gpu(b.gb))
    return _dev_cache[name]


def _same_bits(t, a):
    """Device tensor t against host array a, bit for bit, compared on the device."""
    r = _gpu(a)
    return t.shape == r.shape and t.dtype == r.dtype and bool(torch.equal(t.view(torch.int32), r.view(torch.int32)))


class Crop:
    """A window of frame-sized device tensors [H,W,...] on the host, indexed with the frame's [row, column]."""

    def __init__(self, t, H, window):
        i0, i1, j0, j1 = window
        self.r0, self.c0 = H - 1 - j1, i0
        self.a = t[self.r0:H - j0, i0:i1 + 1].cpu().numpy()

    def __getitem__(self, rc):
        return self.a[rc[0] - self.r0, rc[1] - self.c0]


def _check_windows(name, px, gb, depth=None, bary=None, face=None, label=""):
    """Every window of one frame's device outputs against the statement."""
    case = lf.BY_NAME[name]
    worst = {}
    for window, win in case.windows.items():
        crop = [None if t is None else Crop(t, case.H, win) for t in (px, gb, depth, bary, face)]
        r = lf.check_forward(name, window, *crop, label=label)
        for k in ("depth", "barycentrics", "colours"):
            worst[k] = max(worst.get(k, 0.0), r[k])
    print("%s%s: worst over its windows: %s" % (name, label, worst))


def _setup_launches(fn):
    from dirt_amd import _lib
    _lib.profile_enable(True)
    out = fn()
    torch.cuda.synchronize()
    n = _lib.profile_read()["setup_kernel"][0]
    _lib.profile_enable(False)
    return out, n


@pytest.mark.parametrize("name", [c.name for c in lf.CASES])
def test_forward_whole_frame_and_windows(name):
    import dirt_amd
    from dirt_amd import rasterise_ops
    case = lf.BY_NAME[name]
    b = lf.bulk(name)
    bg, v, c, f, opx, ogb = _device(name)
    px, gb = rasterise_ops._rasterise_batched(bg, v, c, f, None, case.H, case.W, case.C, 0, 0, return_gbuffer=True)
    assert torch.equal(gb, ogb), "g-buffer differs from the oracle's"
    assert torch.equal(px.view(torch.int32), opx.view(torch.int32)), "pixels differ from the oracle's"
    _check_windows(name, px[0], gb[0], label=" (plain raster)")
    g = dirt_amd.rasterise_batch_gbuffer(bg, v, c, f)
    assert torch.equal(g.pixels.view(torch.int32), opx.view(torch.int32))
    assert _same_bits(g.depth, b.depth) and _same_bits(g.barycentrics, b.bary) and _same_bits(g.face_ids, b.face)
    _check_windows(name, g.pixels[0], gb[0], g.depth[0], g.barycentrics[0], g.face_ids[0], label=" (G-buffer raster)")


def _bin_occupancy(sess):
    from dirt_amd import _lib
    B, H, W, C, V, F = sess.dims
    fn = _lib.load().dirt_debug_bin_occupancy
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 4 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p] + \
        [ctypes.POINTER(ctypes.c_uint32)] * 3
    mx, ov, slab = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _lib.check(fn(B, H, W, F, sess.bin_capacity, sess.scratch.data_ptr(), sess.scratch_bytes,
                  torch.cuda.current_stream().cuda_stream, ctypes.byref(mx), ctypes.byref(ov), ctypes.byref(slab)))
    return mx.value, ov.value, slab.value


@pytest.mark.parametrize("name", PATH_CASES)
def test_bin_overflow_in_some_128_px_tiles(name):
    """Slabs of 8 entries: the coarse tiles of the windows (a cluster of 12 faces and more) overflow and filter every
    record themselves, the tiles that see only the frame-sized faces stay binned."""
    from dirt_amd.session import RasteriseSession
    case = lf.BY_NAME[name]
    assert case.cshift == 7
    bg, v, c, f, opx, ogb = _device(name)
    sess = RasteriseSession(1, case.H, case.W, case.C, v.shape[1], f.shape[1], device="cuda",
                            bin_capacity=8 * case.ncoarse)
    sess.forward(bg, v, c, f)
    mx, ov, slab = _bin_occupancy(sess)
    assert slab == 8 and mx > slab and 0 < ov < case.ncoarse, (mx, ov, slab)
    print("%s: %d of %d slabs overflowed, the fullest holds %d entries" % (name, ov, case.ncoarse, mx))
    assert torch.equal(sess.gbuffer, ogb) and torch.equal(sess.pixels.view(torch.int32), opx.view(torch.int32))
    _check_windows(name, sess.pixels[0], sess.gbuffer[0], label=" (bin overflow)")


@pytest.mark.parametrize("name", PATH_CASES)
def test_resolve_only_second_render(name):
    """Two renders of one geometry with sharing on: one setup launch, the second render (other colours and another
    background) is the resolve alone and bit-exact against the oracle."""
    from dirt_amd import rasterise_ops
    case = lf.BY_NAME[name]
    b = lf.bulk(name)
    bg, v, c, f, opx, ogb = _device(name)
    c2 = 1.0 - b.inputs[2]
    bg2 = b.inputs[0][:, ::-1].copy()
    rasterise_ops.workspace_cache_clear(force=True)
    with rasterise_ops.shared_geometry():
        def both():
            first = rasterise_ops._rasterise_batched(bg, v, c, f, None, case.H, case.W, case.C, 0)
            return first, rasterise_ops._rasterise_batched(_gpu(bg2), v, _gpu(c2), f, None, case.H, case.W, case.C, 0,
                                                           0, return_gbuffer=True)
        (first, (px, gb)), n_setup = _setup_launches(both)
    rasterise_ops.workspace_cache_clear(force=True)
    assert n_setup == 1, "the second render of one geometry should run the resolve alone"
    assert torch.equal(first.view(torch.int32), opx.view(torch.int32)) and torch.equal(gb, ogb)
    rpx, rgb, _ = oracle.rasterise_fwd(bg2, b.inputs[1], c2, b.inputs[3])
    assert np.array_equal(rgb, b.gb) and _same_bits(px, rpx)


@pytest.mark.parametrize("name", PATH_CASES)
def test_deep_cull_forced(name):
    from dirt_amd.session import RasteriseSession
    case = lf.BY_NAME[name]
    bg, v, c, f, opx, ogb = _device(name)
    sess = RasteriseSession(1, case.H, case.W, case.C, v.shape[1], f.shape[1], device="cuda", deep_cull=True)
    sess.forward(bg, v, c, f)
    assert torch.equal(sess.gbuffer, ogb) and torch.equal(sess.pixels.view(torch.int32), opx.view(torch.int32))
    _check_windows(name, sess.pixels[0], sess.gbuffer[0], label=" (deep cull)")


@pytest.mark.parametrize("name", PATH_CASES)
def test_few_faces_are_not_routed_to_the_fused_raster(name):
    """F = 32 is the fused small-scene raster's face limit, but it also needs at most 8192 tiles (raster_kernel.h
    kFusedMaxTiles): these frames have 66049 and 262144, so the setup + binned path runs (one setup launch).  The last
    32 faces of the scene: the coarse-tile straddlers, the frame-sized pair, the clipped face, a tie and a cluster."""
    from dirt_amd import rasterise_ops
    case = lf.BY_NAME[name]
    b = lf.bulk(name)
    assert lf.layout(case.W, case.H)[4] > 8192
    bg, v, c, f, _, _ = _device(name)
    f32 = b.inputs[3][:, -32:]
    (px, gb), n_setup = _setup_launches(lambda: rasterise_ops._rasterise_batched(
        bg, v, c, _gpu(f32), None, case.H, case.W, case.C, 0, 0, return_gbuffer=True))
    assert n_setup == 1
    rpx, rgb, _ = oracle.rasterise_fwd(b.inputs[0], b.inputs[1], b.inputs[2], f32)
    assert (rgb >= 0).any() and _same_bits(gb, rgb) and _same_bits(px, rpx)


def test_oceanic_horizon_8192x2049():
    """Against the oracle alone (no independent statement of the procedural programs exists)."""
    from dirt_amd import rasterise_ops
    from test_oceanic_oracle import CAMS, fullscreen
    H, W = 2049, 8192
    bg, v, c, f = fullscreen(H, W)
    cam = CAMS["square_test"]
    px, gb = rasterise_ops._rasterise_batched(*(_gpu(a) for a in (bg, v, c, f)),
                                              torch.tensor(cam, dtype=torch.float32).cuda(), H, W, bg.shape[3], 1,
                                              return_gbuffer=True)
    rpx, rgb, _ = oracle.rasterise_fwd(bg, v, c, f, shader_id=1, camera_pos=np.array(cam, np.float32))
    assert _same_bits(gb, rgb) and _same_bits(px, rpx)


def test_hill_8192x2049():
    """Against the oracle alone (no independent statement of the procedural programs exists)."""
    from test_gpu_oceanic import _hill_gpu
    from test_procedural_oracle import HILL_CAMS, hill_cam
    H, W = 2049, 8192
    v, f = scenes.fullscreen_quad()
    # (a 257x1024 terrain, every texel repeated 8x8: building the full-size one takes longer than the render)
    T = np.ascontiguousarray(np.repeat(np.repeat(scenes.hill_terrain(257, 1024, 4), 8, 0), 8, 1)[None, :H])
    cam = hill_cam(HILL_CAMS["harness"])
    px, gb = _hill_gpu(T, v[None], f[None], 3, cam)
    rpx, rgb, _ = oracle.hill_fwd(T, v[None], f[None], 3, cam)
    np.testing.assert_array_equal(gb, rgb)
    np.testing.assert_array_equal(px, rpx)


def _forward_with_grad(name):
    from dirt_amd import rasterise_ops
    case = lf.BY_NAME[name]
    bg, v, c, f, opx, ogb = _device(name)
    leaves = [t.detach().requires_grad_(True) for t in (bg, v, c)]
    px, gb = rasterise_ops._rasterise_batched(*leaves, f, None, case.H, case.W, case.C, 0, 0, return_gbuffer=True)
    # the statement reads the oracle's g-buffer and pixels: the GPU's must be the same
    assert torch.equal(gb, ogb) and torch.equal(px.detach().view(torch.int32), opx.view(torch.int32))
    return px, leaves, ogb


@pytest.mark.parametrize("name,window", lf.PAIRS, ids=["%s-%s" % p for p in lf.PAIRS])
def test_backward_windows_within_the_bound(name, window):
    ref = lf.reference(name, window)
    px, leaves, ogb = _forward_with_grad(name)
    gp = _gpu(lf.cotangent(name, window))
    gbg, gv, gc = torch.autograd.grad(px, leaves, gp)
    want = torch.where((ogb < 0)[..., None], gp, torch.zeros_like(gp))
    assert torch.equal(gbg.view(torch.int32), want.view(torch.int32)), "grad_background"
    gv, gc = gv.cpu().numpy(), gc.cpu().numpy()
    assert np.all(gv[..., 2] == 0.0)
    print("\n" + bc.fmt("%s %s" % (name, window), bc.check_bound(gv, gc, ref)))


def _tiles_spanned(v, f, W, H):
    """Per face, an upper bound of the 16x16 tiles it touches: its area and twice its perimeter in tiles."""
    p = (v[:, :2] / v[:, 3:4] + 1.0) * (np.array([W, H]) / 2.0)
    a, b, c = (p[f[:, k]].astype(np.float64) for k in range(3))
    area = 0.5 * np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))
    perimeter = sum(np.linalg.norm(x - y, axis=1) for x, y in ((a, b), (b, c), (c, a)))
    return area / 256.0 + perimeter / 8.0


@pytest.mark.parametrize("name", DENSE_CASES)
def test_dense_backward_against_the_oracle(name):
    """A dense standard-normal cotangent, one frame size each, against the oracle under the strict pair -- on the
    case's scene without its last three faces (the two that cover the whole frame and the clipped one that reaches
    from the centre past the far corner).

    Why without them.  The strict pair allows grad_vertex_colors 1e-5 |ref| + 1e-6 scale.  The kernel adds one float32
    atomic per tile and record to an element, each rounding at the running sum's ulp; under a zero-mean cotangent the
    running sum is at least as large as the result, so T tiles leave sqrt(T / 3) 2^-24 of it or more: 0.6e-5 for
    the 2^15 tiles of a face covering half of 4096x4096, 1.25e-5 for the 2^17 of 8192x8192 -- at the tolerance by the
    number format alone, for any summation by float32 atomics -- and at most 0.45e-5 at T = 2^14.  With the
    frame-sized faces in the scene their six colour elements landed at 0.4 to 1.7 of the tolerance, a different one
    over in four of five runs on an MI355X, while the error was 0.1 u S of the per-element contract that the windows
    hold the kernel to.  So this scale-relative contract is stated on faces of at most 2^14 tiles (asserted from the
    geometry: area plus twice the perimeter; the largest here spans about 10,500): every remaining face of the scene,
    the 300 to 3000 px ones included, with every tile of the frame still run by the raster and the backward and
    grad_background compared over all of it.  The
    frame-sized and clipped faces keep their per-element checks in test_backward_windows_within_the_bound.
    Measured on an MI355X in seven runs: grad_vertex_colors at most 0.80 of the tolerance (4097x4097, 0.36 to 0.80; the
    other sizes at most 0.60), grad_vertices at most 0.08."""
    case = lf.BY_NAME[name]
    b = lf.bulk(name)
    bg, v, c, f = b.inputs
    f = np.ascontiguousarray(f[:, :-3])
    spans = _tiles_spanned(v[0], f[0], case.W, case.H)
    assert 1 << 12 <= spans.max() <= 1 << 14, spans.max()
    from dirt_amd import rasterise_ops
    rpx, rgb, _ = oracle.rasterise_fwd(bg, v, c, f)
    dbg, dv, dc, _, _, _ = _device(name)
    leaves = [t.detach().requires_grad_(True) for t in (dbg, dv, dc)]
    px, gb = rasterise_ops._rasterise_batched(*leaves, _gpu(f), None, case.H, case.W, case.C, 0, 0, return_gbuffer=True)
    assert _same_bits(gb, rgb) and _same_bits(px.detach(), rpx)
    gp = np.random.default_rng(7).standard_normal(rpx.shape, dtype=np.float32)
    gbg, gv, gc = torch.autograd.grad(px, leaves, _gpu(gp))
    rgv, rgc, rgbg = oracle.rasterise_bwd(v, c, f, rpx, gp, rgb)
    assert _same_bits(gbg, rgbg)
    gv, gc = gv.cpu().numpy(), gc.cpu().numpy()
    assert np.all(gv[..., 2] == 0.0)
    for what, got, want in (("grad_vertex_colors", gc, rgc), ("grad_vertices", gv, rgv)):
        rtol, atol_rel = STRICT[what]
        err, scale = np.abs(got.astype(np.float64) - want), float(np.abs(want).max())
        ratio = err / (rtol * np.abs(want) + atol_rel * scale)
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        print("%s %s: worst error / tolerance %.3f at %s (error %.3g, oracle %.6g, scale %.6g), %d of %d over" % (
            name, what, ratio[at], at, err[at], want[at], scale, (ratio > 1).sum(), ratio.size))
    assert_close_grad(gc, rgc, "grad_vertex_colors", strict=True)
    assert_close_grad(gv, rgv, "grad_vertices", strict=True)


@pytest.mark.parametrize("name,window", lf.SINGLE_PAIRS, ids=[p[1] for p in lf.SINGLE_PAIRS])
def test_large_edge_single_term(name, window):
    """DESIGN.md 5, the int64 edge path: a single pair term whose midpoint lies within 1/256 px of an edge of
    2021 px, E_k >= 2^24 at the owner's pixel and |E2_k| <= E_k / 64 (asserted by the case).  grad_kernel.h converts
    E_k before it forms the midpoint value, so the conversion's error is relative to E_k, not to the term: the
    kernel's bound carries the allowance 2 u L for terms on that path (tests/backward_cases.py).  Measured on an
    MI355X: 1.9 to 4.7 times the bound without the allowance on seven of the eight windows (0.59 on the eighth), at
    most 0.13 of the bound with it; printed for the record."""
    ref = lf.reference(name, window)
    px, leaves, ogb = _forward_with_grad(name)
    gp = _gpu(lf.cotangent(name, window))
    gbg, gv, gc = torch.autograd.grad(px, leaves, gp)
    want = torch.where((ogb < 0)[..., None], gp, torch.zeros_like(gp))
    assert torch.equal(gbg.view(torch.int32), want.view(torch.int32)), "grad_background"
    gv = gv.cpu().numpy()
    vk, axis, _ = lf.SINGLE.vertex[window]
    err = abs(float(gv[0, vk, axis]) - ref.gv[0, vk, axis])
    print("\n%s: the single-term element: %.2f of the bound without the int64 allowance" % (
        window, err / (ref.bound_vertices()[0, vk, axis] - 2 * bc.U * ref.L_v[0, vk, axis])))
    print(bc.fmt(window, bc.check_bound(gv, gc.cpu().numpy(), ref)))


def test_offsets_past_2_31():
    """B, H, W, C = 17, 4096, 4096, 8: frame 16 starts at element 2^31 exactly, the smallest shape whose element
    offsets (pixels, background, grad_pixels, grad_background) do not fit a signed 32-bit index in the setup, raster
    and grad kernels.  The frames differ, so a wrapped offset lands on visibly different data: every frame has its
    own background level and vertex colours, and the geometry of frames 15 and 16 is shifted.  3000 faces of up to
    64 px around their centres per frame (the suite's standard random scene, which the strict pair is held on).
    Forward: frames 0, 15 and 16 against the oracle, one frame at a time on the host; every frame's uncovered pixels
    equal its own background, on the device; the far-corner window of frame 16 against the exact statement.
    Backward (the background is freed first: at most three 9.1 GB tensors are alive at once, no full-size
    temporaries, and the allocator's blocks are released at the end): frames 0 and 16 strictly against the oracle,
    grad_background on the device for every frame.  The pixel-index threshold, B * H * W >= 2^31, is left out: the
    g-buffer alone would take 8.6 GB and pixels of one channel as much again four times over.  Wall time on an
    MI355X: DESIGN.md 5."""
    import forward_exact
    from dirt_amd import _lib
    B, H, W, C = 17, 4096, 4096, 8
    assert 16 * H * W * C == 2 ** 31
    _dev_cache.clear()
    rng = np.random.default_rng(31)
    # (radius 1 px of a 64x64 frame = 64 px of this one; its background is not used)
    _, v0, _, f0 = scenes.random_triangles(F=3000, W=64, H=64, C=C, radius_px=1.0, seed=31, perspective=True)
    # ... and a cluster of 12 faces (16 px) in the last 40 pixels of both axes, in every frame: the far corner
    cl = 1.0 - rng.uniform(0, 40, (12, 1, 2)) / 2048.0 + rng.uniform(-16, 16, (12, 3, 2)) / 2048.0
    cl = np.concatenate([cl, rng.uniform(-0.9, 0.9, (12, 1, 1)) + np.zeros((12, 3, 1)), np.ones((12, 3, 1))], -1)
    v = np.repeat(v0[None], B, 0)
    v[15, :, 0] += 0.013 * v[15, :, 3]
    v[16, :, 1] -= 0.021 * v[16, :, 3]
    v = np.concatenate([v, np.repeat(cl.reshape(1, 36, 4).astype(np.float32), B, 0)], 1)
    f0 = np.arange(v.shape[1], dtype=np.int32).reshape(-1, 3)
    V, F = v.shape[1], f0.shape[0]
    f = np.repeat(f0[None], B, 0)
    c = rng.uniform(0, 1, (B, V, C)).astype(np.float32)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    saved_b, scratch_b = _lib.workspace_sizes(B, H, W, C, V, F, 0)
    try:
        bg = torch.rand((B, H, W, C), device="cuda")
        for b in range(B):
            bg[b].mul_(0.03125).add_(b / 32.0)  # frame b: [b / 32, (b + 1) / 32)
        px = torch.empty_like(bg)
        gb = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
        saved = torch.empty(saved_b, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(scratch_b, dtype=torch.uint8, device="cuda")
        vt, ct, ft = _gpu(v), _gpu(c), _gpu(f)
        _lib.check(lib.dirt_rasterise_fwd(
            bg.data_ptr(), vt.data_ptr(), ct.data_ptr(), ft.data_ptr(), None, B, H, W, C, V, F, _lib.SHADER_GOURAUD,
            px.data_ptr(), gb.data_ptr(), saved.data_ptr(), saved_b, scratch.data_ptr(), scratch_b, 0, 0, None, None,
            stream))
        for b in range(B):
            hole = (gb[b] < 0)[..., None]
            assert 0 < int(hole.sum()) < H * W, b
            assert torch.equal(torch.where(hole, px[b], 0.0).view(torch.int32),
                               torch.where(hole, bg[b], 0.0).view(torch.int32)), "frame %d: background" % b
        host = {}
        for b in (0, 15, 16):
            s = slice(b, b + 1)
            rpx, rgb, _ = oracle.rasterise_fwd(bg[s].cpu().numpy(), v[s], c[s], f[s])
            assert _same_bits(gb[s], rgb) and _same_bits(px[s], rpx), "frame %d" % b
            host[b] = (rpx, rgb)
        win = (W - lf.WW, W - 1, H - lf.WH, H - 1)
        fr = forward_exact.Frame(v[16], f[16], W, H, window=win)
        r = forward_exact.check_frame(fr, Crop(bg[16], H, win), c[16], Crop(px[16], H, win), Crop(gb[16], H, win))
        print("frame 16, far corner: %s" % r)
        assert r["covered"] > 0 and r["share"] <= 0.02
        del bg, hole
        gp = torch.randn((B, H, W, C), device="cuda")
        gbg = torch.empty_like(gp)
        gv = torch.empty((B, V, 4), device="cuda")
        gc = torch.empty((B, V, C), device="cuda")
        _lib.check(lib.dirt_rasterise_bwd(
            vt.data_ptr(), ct.data_ptr(), ft.data_ptr(), px.data_ptr(), gp.data_ptr(), gb.data_ptr(), saved.data_ptr(),
            B, H, W, C, V, F, gv.data_ptr(), gc.data_ptr(), gbg.data_ptr(), 0, stream))
        for b in range(B):
            want = torch.where((gb[b] < 0)[..., None], gp[b], 0.0)
            assert torch.equal(gbg[b].view(torch.int32), want.view(torch.int32)), "frame %d: grad_background" % b
        del want
        gv, gc = gv.cpu().numpy(), gc.cpu().numpy()
        assert np.all(gv[..., 2] == 0.0)
        for b in (0, 16):
            s = slice(b, b + 1)
            rgv, rgc, _ = oracle.rasterise_bwd(v[s], c[s], f[s], host[b][0], gp[s].cpu().numpy(), host[b][1])
            assert_close_grad(gc[s], rgc, "grad_vertex_colors frame %d" % b, strict=True)
            assert_close_grad(gv[s], rgv, "grad_vertices frame %d" % b, strict=True)
    finally:
        bg = px = gb = gp = gbg = saved = scratch = None
        torch.cuda.empty_cache()



def _tiny_batch(B, seed=3):
    """B frames of 4x4 pixels, one channel, one face each, every frame its own."""
    rng = np.random.default_rng(seed)
    v = np.tile(np.array([[-0.9, -0.8, 0.1, 1.0], [0.9, -0.6, 0.2, 1.0], [-0.1, 0.9, 0.3, 1.0]], np.float32), (B, 1, 1))
    v[..., :2] += rng.uniform(-0.35, 0.35, (B, 3, 2)).astype(np.float32)
    return (rng.uniform(0, 1, (B, 4, 4, 1)).astype(np.float32), v, rng.uniform(0, 1, (B, 3, 1)).astype(np.float32),
            np.tile(np.arange(3, dtype=np.int32), (B, 1, 1)))


def test_batch_beyond_16_bits_of_grid_y():
    """B is grid.y of the setup, raster and grad launches (dim3(..., B)), and validate() admits any B with
    B * F < 2^28; nothing else in the suite renders more than 64 frames.  65537 frames of 4x4 pixels, F = 1, C = 1,
    every frame its own triangle: all frames bit-exact against the oracle, forward and grad_background, and the last
    frame's backward (block 65536 of grid.y) under the per-element bound.
    The device's limit is read from its attribute through the library, and the branch is stated: an MI355X reports
    hipDeviceAttributeMaxGridDimY = 65536, so B = 65537 is past what the attribute admits -- and the launches run
    all the same, as the 70,000-frame vertex-normal launch of tests/test_gpu_lighting_f64.py does.  The attribute
    is not the launch limit of this runtime, which is why validate() holds no batch to it."""
    from dirt_amd import _lib
    from dirt_amd.session import RasteriseSession
    lib = _lib.load()
    lib.dirt_debug_max_grid_y.restype = ctypes.c_int
    lib.dirt_debug_max_grid_y.argtypes = []
    torch.cuda.current_device()  # (the runtime is up and the device current)
    lim = lib.dirt_debug_max_grid_y()
    B = 65537
    print("hipDeviceAttributeMaxGridDimY = %d: B = %d is %s what it admits" % (
        lim, B, "within" if B <= lim else "past"))
    assert lim >= 65535
    inputs = _tiny_batch(B)
    rpx, rgb, _ = oracle.rasterise_fwd(*inputs)
    assert len({rgb[b].tobytes() for b in range(0, B, 997)}) > 8 and (rgb[-1] >= 0).any()  # (the frames differ)
    sess = RasteriseSession(B, 4, 4, 1, 3, 1, device="cuda")
    sess.forward(*(_gpu(a) for a in inputs))
    assert _same_bits(sess.gbuffer, rgb) and _same_bits(sess.pixels, rpx)
    gp = np.random.default_rng(4).standard_normal(rpx.shape).astype(np.float32)
    gbg, gv, gc = sess.backward(_gpu(gp))
    assert _same_bits(gbg, np.where((rgb < 0)[..., None], gp, np.float32(0.0)))
    last = slice(B - 1, B)
    ref = bc.Reference([a[last] for a in inputs], 0, forward=(rpx[last], rgb[last]), grad_pixels=gp[last])
    assert ref.n_v.sum() > 0 and ref.n_c.sum() > 0
    print(bc.fmt("B = %d, last frame" % B, bc.check_bound(gv[last].cpu().numpy(), gc[last].cpu().numpy(), ref)))
