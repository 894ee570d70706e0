"""GPU: dirt_rasterise_fwd_resolve (ABI 13) through the raw C ABI against the CPU oracle.

The resolve serves a render that shares its geometry with an earlier Gouraud forward: it reads that forward's g-buffer
and `saved` records and runs raster_kernel's RESOLVE instantiation alone.  The full forward is pinned to the oracle at
every shape and path of tests/test_gpu_parity.py; these tests hold the resolve to the same oracle in the same
situations -- every channel specialisation (1, 3, 7, generic), batches, clipped sub-triangle records, the int32 /
int64 edge paths, `saved` written by the fused, the overflowed-bin and the occluder-culling forwards, frames smaller
than a tile and 8192 wide, non-finite backgrounds, its own zero-fill of the gradient accumulators, and the backward
that reads a `saved` shared between renders of different channel counts.

Flow of every case (`_check`): one dirt_rasterise_fwd at C1; for each (background, colours) of the case one
dirt_rasterise_fwd_resolve on that forward's g-buffer and saved records; then, in the reverse order of the resolves,
one dirt_rasterise_bwd per render with the render's own g-buffer copy and the shared `saved`.  Pixels, g-buffer and
grad_background are bit-exact; grad_vertices and grad_vertex_colors meet the suite's contract
(test_gpu_parity.assert_close_grad; `strict` where the full forward's test is strict); the first forward's g-buffer
and `saved` are byte-identical afterwards (the header: "only read").  A case with a precondition asserts it from the
oracle's g-buffer, so a scene that stops reaching its path fails instead of passing vacuously."""
import glob
import os

import numpy as np
import pytest
import torch

import scenes
from oracle import oracle
from test_gpu_parity import GOLDEN, assert_close_grad, _gpu

pytestmark = pytest.mark.gpu

MULTI = 1 << 30  # kGbufMulti: the visible record belongs to a clipped face


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _batched(scene):
    return scene if scene[0].ndim == 4 else tuple(a[None] for a in scene)


class _FirstForward:
    """One dirt_rasterise_fwd on (bg1, v, c1, f): its g-buffer and `saved`, with clones taken right after it."""

    def __init__(self, bg1, v, c1, f, bin_capacity=0, flags=0):
        from dirt_amd import _lib
        self.v, self.f = v, f
        B, H, W, C1 = bg1.shape
        self.B, self.H, self.W, self.V, self.F = B, H, W, v.shape[1], f.shape[1]
        self.vt, self.ft = _gpu(v), _gpu(f)
        bt, ct = _gpu(bg1), _gpu(c1)
        self.saved_bytes, scratch_b = _lib.workspace_sizes(B, H, W, C1, self.V, self.F, bin_capacity)
        self.saved = torch.zeros(max(self.saved_bytes, 1), dtype=torch.uint8, device="cuda")
        scratch = torch.zeros(max(scratch_b, 1), dtype=torch.uint8, device="cuda")
        self.pixels = torch.empty((B, H, W, C1), device="cuda")
        self.gbuffer = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().dirt_rasterise_fwd(
            bt.data_ptr(), self.vt.data_ptr(), ct.data_ptr(), self.ft.data_ptr(), None, B, H, W, C1, self.V, self.F, 0,
            self.pixels.data_ptr(), self.gbuffer.data_ptr(), self.saved.data_ptr(), self.saved_bytes,
            scratch.data_ptr(), scratch_b, bin_capacity, flags, None, None, _stream()))
        torch.cuda.synchronize()
        self.saved0, self.gbuffer0 = self.saved.clone(), self.gbuffer.clone()

    def resolve(self, bg2, c2, zero_v=None, zero_c=None):
        """dirt_rasterise_fwd_resolve over (bg2, c2): (background, colours, pixels, g-buffer copy) on the device."""
        from dirt_amd import _lib
        C2 = bg2.shape[-1]
        assert bg2.shape == (self.B, self.H, self.W, C2) and c2.shape == (self.B, self.V, C2)
        bt, ct = _gpu(bg2), _gpu(c2)
        px = torch.empty((self.B, self.H, self.W, C2), device="cuda")
        gb = torch.full((self.B, self.H, self.W), -7, dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().dirt_rasterise_fwd_resolve(
            bt.data_ptr(), ct.data_ptr(), self.B, self.H, self.W, C2, self.V, self.F, self.gbuffer.data_ptr(),
            self.saved.data_ptr(), self.saved_bytes, px.data_ptr(), gb.data_ptr(),
            zero_v.data_ptr() if zero_v is not None else None, zero_c.data_ptr() if zero_c is not None else None,
            _stream()))
        return bt, ct, px, gb

    def backward(self, ct, px, gb, gp, gv=None, gc=None, flags=0, want=(True, True)):
        """dirt_rasterise_bwd of a resolved render: its own g-buffer copy, the shared saved records."""
        from dirt_amd import _lib
        C2 = px.shape[-1]
        if gv is None and want[0]:
            gv = torch.full((self.B, self.V, 4), 7.0, device="cuda")
        if gc is None and want[1]:
            gc = torch.full((self.B, self.V, C2), 7.0, device="cuda")
        gbg = torch.full((self.B, self.H, self.W, C2), 7.0, device="cuda")
        gt = _gpu(gp)
        _lib.check(_lib.load().dirt_rasterise_bwd(
            self.vt.data_ptr(), ct.data_ptr(), self.ft.data_ptr(), px.data_ptr(), gt.data_ptr(), gb.data_ptr(),
            self.saved.data_ptr(), self.B, self.H, self.W, C2, self.V, self.F,
            gv.data_ptr() if gv is not None else None, gc.data_ptr() if gc is not None else None, gbg.data_ptr(),
            flags, _stream()))
        torch.cuda.synchronize()
        return gbg, gv, gc

    def assert_only_read(self):
        torch.cuda.synchronize()
        assert torch.equal(self.saved, self.saved0), "a resolve or backward wrote the shared saved records"
        assert torch.equal(self.gbuffer, self.gbuffer0), "a resolve or backward wrote the first forward's g-buffer"


def _render_inputs(shape_bhw, V, C2, seed):
    """Fresh colours (signed) and background of a resolved render, from its own seed."""
    rng = np.random.default_rng(seed)
    B, H, W = shape_bhw
    return (rng.uniform(0, 1, (B, H, W, C2)).astype(np.float32), rng.uniform(-1, 1, (B, V, C2)).astype(np.float32))


def _check(first, renders, seed, strict=False, f64=False):
    """Resolve every (bg2, c2) of `renders` on `first`, then run their backwards in reverse order; compare each with
    the oracle (f64: gradients against tests/backward_f64.py instead).  Returns the oracle's g-buffer."""
    v, f = first.v, first.f
    outs = []
    for bg2, c2 in renders:
        outs.append(first.resolve(bg2, c2))
    torch.cuda.synchronize()
    ref_gb = None
    refs = []
    for k, (bg2, c2) in enumerate(renders):
        px, gb, _ = oracle.rasterise_fwd(bg2, v, c2, f)
        refs.append(px)
        ref_gb = gb
        np.testing.assert_array_equal(outs[k][2].cpu().numpy(), px)  # bit-exact; non-finite values in place
        got_gb = outs[k][3].cpu().numpy()
        np.testing.assert_array_equal(got_gb, gb)  # (multi bit included)
        np.testing.assert_array_equal(got_gb, first.gbuffer0.cpu().numpy())
    for k in reversed(range(len(renders))):
        bg2, c2 = renders[k]
        gp = np.random.default_rng(seed * 100 + k).standard_normal(bg2.shape).astype(np.float32)
        _, ct, px, gb = outs[k]
        gbg, gv, gc = (t.cpu().numpy() for t in first.backward(ct, px, gb, gp))
        if f64:
            import backward_f64
            rgv, rgc, rgbg = backward_f64.backward_batch(v, f, refs[k], gp, ref_gb)
            rgbg = rgbg.astype(np.float32)
        else:
            rgv, rgc, rgbg = oracle.rasterise_bwd(v, c2, f, refs[k], gp, ref_gb)
        np.testing.assert_array_equal(gbg, rgbg)
        assert_close_grad(gc, rgc, "grad_vertex_colors render %d (C=%d)" % (k, bg2.shape[-1]), strict)
        assert_close_grad(gv, rgv, "grad_vertices render %d (C=%d)" % (k, bg2.shape[-1]), strict)
        assert np.all(gv[..., 2] == 0.0)
    first.assert_only_read()
    return ref_gb


def _case(scene, channels, seed, bin_capacity=0, flags=0, strict=False, f64=False):
    bg1, v, c1, f = _batched(scene)
    first = _FirstForward(bg1, v, c1, f, bin_capacity, flags)
    renders = [_render_inputs(bg1.shape[:3], v.shape[1], C2, seed * 1000 + C2) for C2 in channels]
    gb = _check(first, renders, seed, strict, f64)
    return first, gb


def _covered(gb):
    return gb >= 0


def _record(gb):
    return gb & ~MULTI


# ---- case 1: every channel count (the four specialisations: 1, 3, 7, generic) over one 3-channel forward


def test_resolve_every_channel_count():
    _, gb = _case(scenes.random_triangles(F=400, W=67, H=45, radius_px=9.0, seed=0), range(1, 9), seed=1)
    cov = int(_covered(gb).sum())
    assert 0 < cov < gb.size, "covered and background pixels must both be present (%d of %d)" % (cov, gb.size)


# ---- case 2: records of clipped sub-triangles (kGbufMulti, record index >= F, the record's own 1/w)


@pytest.mark.parametrize("name", ["clipping", "near_w0"])
def test_resolve_clipped_sub_triangle_records(name):
    scene = scenes.clipping_scene() if name == "clipping" else scenes.near_w0_scene(3)
    F = scene[3].shape[0]
    assert F > 32  # binned, not fused
    _, gb = _case(scene, (1, 5, 7), seed=2)
    cov = _covered(gb)
    assert (cov & ((gb & MULTI) != 0)).any(), "no visible record of a clipped face"
    assert (cov & (_record(gb) >= F)).any(), "no visible extra sub-triangle record (index >= F)"


# ---- case 3: `saved` published by the fused small-scene forward (tile 0 of each frame writes it)


@pytest.mark.parametrize("s", range(6))
def test_resolve_after_fused_forward(s):
    scene = scenes.adversarial_scene(s, W=33, H=17, C=3, F=8)
    F = scene[3].shape[0]
    assert F <= 32
    _, gb = _case(scene, ((3, 1, 7, 5)[s % 4],), seed=30 + s)
    cov = _covered(gb)
    if s in (0, 1, 2, 5):
        assert (cov & ((gb & MULTI) != 0)).any(), "seed %d should show a clipped face's record" % s
    else:
        assert cov.any() and not cov.all(), "seed %d should be partly covered" % s


def test_resolve_after_fused_forward_batch():
    W, H, C = 33, 17, 3
    frames = [scenes.adversarial_scene(20 + k, W=W, H=H, C=C, F=8) for k in range(3)]
    F = max(fr[3].shape[0] for fr in frames)
    frames = [(bg, v, c, np.concatenate([f, np.zeros((F - f.shape[0], 3), np.int32)])) for bg, v, c, f in frames]
    V = max(fr[1].shape[0] for fr in frames)
    frames = [(bg, np.concatenate([v, np.tile(v[:1], (V - v.shape[0], 1))]),
               np.concatenate([c, np.tile(c[:1], (V - c.shape[0], 1))]), f) for bg, v, c, f in frames]
    scene = tuple(np.stack([fr[k] for fr in frames]) for k in range(4))
    assert scene[3].shape[1] <= 32
    _, gb = _case(scene, (7,), seed=36)
    assert all(_covered(gb[b]).any() for b in range(3))


# ---- cases 4, 5: `saved` of a forward whose slabs overflowed (all of them; some of them)


def test_resolve_after_every_slab_overflowed():
    _case(scenes.random_triangles(F=800, W=128, H=96, radius_px=14.0, seed=4), (1, 7), seed=4, bin_capacity=64)


def test_resolve_after_some_slabs_overflowed():
    bg, v, c, f = scenes.random_triangles(F=600, W=128, H=96, radius_px=6.0, seed=11)
    v = v.copy()
    v[:400 * 3, :2] = v[:400 * 3, :2] * 0.3 - 0.6
    v[400 * 3 + 2, 3] = -0.5
    _case((bg, v, c, f), (3,), seed=5, bin_capacity=1000)


# ---- case 6: large triangles (edges past 64 px: the int64 edge path), after the occluder-culling forward and the
# plain one


def test_resolve_large_triangles_after_deep_cull_on_and_off():
    from dirt_amd import _lib
    scene = scenes.random_triangles(F=60, W=200, H=150, radius_px=120.0, seed=11)
    firsts = [_case(scene, (3, 8), seed=6, flags=flags)[0] for flags in (_lib.FWD_DEEP_CULL, _lib.FWD_DEEP_CULL_OFF)]
    assert torch.equal(firsts[0].gbuffer0, firsts[1].gbuffer0)
    assert torch.equal(firsts[0].pixels, firsts[1].pixels)


# ---- case 7: degenerate, out-of-range and non-finite faces (culled by the first forward)


def test_resolve_degenerate_and_out_of_range_faces():
    bg, v, c, f = scenes.random_triangles(F=200, W=64, H=64, radius_px=10.0, seed=9)
    f = f.copy()
    f[3] = [5, 5, 5]
    f[7] = [0, 1, 10 ** 6]
    f[8] = [-1, 2, 3]
    v = v.copy()
    v[30, 0] = np.nan
    _case((bg, v, c, f), (1, 3), seed=7)


# ---- case 8: frame offsets into recs, fdata, gbuffer_in, colours and backgrounds for B > 1


def test_resolve_batch_of_frames():
    scene = scenes.batch_of(scenes.random_triangles, 3, F=500, W=96, H=80, radius_px=10.0, seed=20)
    _, gb = _case(scene, (3, 7), seed=8)
    for b in range(3):
        assert _covered(gb[b]).sum() > 5000
    assert not np.array_equal(gb[0], gb[1]) and not np.array_equal(gb[1], gb[2])


# ---- case 9: frames smaller than a tile or a coarse tile, odd sizes


@pytest.mark.parametrize("H,W", [(1, 1), (1, 17), (17, 1), (15, 15), (16, 33), (65, 63)])
def test_resolve_tiny_and_odd_frames(H, W):
    for C1, C2 in ((3, 1), (1, 3)):
        _case(scenes.random_triangles(F=60, W=W, H=H, C=C1, radius_px=max(2.0, min(W, H) / 2.0),
                                      seed=H * 100 + W + C1), (C2,), seed=H * 100 + W)


# ---- case 10: DIRT_MAX_DIM along each axis


@pytest.mark.parametrize("H,W", [(40, 8192), (8192, 24)])
def test_resolve_maximum_frame_dimensions(H, W):
    _case(scenes.random_triangles(F=3000, W=W, H=H, radius_px=10.0, seed=12), (3,), seed=10)


# ---- case 11: dense tiles (the backward's slot table and tail overflow) behind a resolve of another channel count


def test_resolve_dense_tiles():
    bg, v, c, f = scenes.random_triangles(F=30000, W=64, H=48, C=7, radius_px=1.0, seed=17)
    _, gb = _case((bg, v, c, f), (3,), seed=11)
    g = gb[0]
    per_tile = [len(np.unique(g[y:y + 16, x:x + 16][g[y:y + 16, x:x + 16] >= 0]))
                for y in range(0, 48, 16) for x in range(0, 64, 16)]
    assert max(per_tile) > 64


# ---- case 12: non-finite backgrounds


@pytest.mark.parametrize("fill", [-np.inf, np.inf, np.nan], ids=["neg_inf", "pos_inf", "nan"])
def test_resolve_non_finite_background(fill):
    bg1, v, c1, f = _batched(scenes.random_triangles(F=400, W=67, H=45, radius_px=9.0, seed=0))
    first = _FirstForward(bg1, v, c1, f)
    renders = []
    for C2 in (3, 7):
        _, c2 = _render_inputs(bg1.shape[:3], v.shape[1], C2, 12000 + C2)
        renders.append((np.full(bg1.shape[:3] + (C2,), fill, np.float32), c2))
    gb = _check(first, renders, seed=12)
    assert 0 < _covered(gb).sum() < gb.size


# ---- case 13: no faces at all


def test_resolve_without_faces():
    bg1, v, c1, f = _batched(scenes.random_triangles(F=10, W=32, H=32, seed=1))
    f = f[:, :0]
    first = _FirstForward(bg1, v, c1, f)
    bg2, c2 = _render_inputs(bg1.shape[:3], v.shape[1], 3, 13)
    V = v.shape[1]
    zv, zc = torch.full((1, V, 4), 7.0, device="cuda"), torch.full((1, V, 3), 7.0, device="cuda")
    assert (V * 3) % 4 != 0  # the vectorised zero-fill leaves a scalar tail
    _, ct, px, gb = first.resolve(bg2, c2, zv, zc)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(px.cpu().numpy(), bg2)
    assert torch.count_nonzero(zv).item() == 0 and torch.count_nonzero(zc).item() == 0
    assert (gb == -1).all().item()
    gp = np.random.default_rng(13).standard_normal(bg2.shape).astype(np.float32)
    gbg, gv, gc = first.backward(ct, px, gb, gp)
    np.testing.assert_array_equal(gbg.cpu().numpy(), gp)
    assert torch.count_nonzero(gv).item() == 0 and torch.count_nonzero(gc).item() == 0
    _check(first, [(bg2, c2)], seed=13)


# ---- case 14: the committed fixtures (no oracle call)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))), ids=os.path.basename)
def test_resolve_golden_fixtures(path):
    z = np.load(path)
    bg, v, c, f = z["background"], z["vertices"], z["vertex_colors"], z["faces"]
    C = bg.shape[-1]
    # the first forward renders other colours (another channel count where the fixture's is 3)
    bg1, c1 = _render_inputs(bg.shape[:3], v.shape[1], 1 if C == 3 else 3, 14)
    first = _FirstForward(bg1, v, c1, f)
    np.testing.assert_array_equal(first.gbuffer0.cpu().numpy(), z["gbuffer"])
    _, ct, px, gb = first.resolve(bg, c)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gb.cpu().numpy(), z["gbuffer"])
    np.testing.assert_array_equal(px.cpu().numpy(), z["pixels"])
    gbg, gv, gc = (t.cpu().numpy() for t in first.backward(ct, px, gb, z["grad_pixels"]))
    np.testing.assert_array_equal(gbg, z["grad_background"])
    assert_close_grad(gc, z["grad_vertex_colors"], "grad_vertex_colors", strict=True)
    assert_close_grad(gv, z["grad_vertices"], "grad_vertices", strict=True)
    assert np.all(gv[..., 2] == 0.0)
    first.assert_only_read()


# ---- case 15: clipped slivers against the independent float64 backward, strict


@pytest.mark.parametrize("s", range(10))
def test_resolve_clipped_slivers_vs_float64(s):
    _case(scenes.clipped_sliver_scene(s), (3,), seed=150 + s, strict=True, f64=True)


# ---- the resolve's own zero-fill of the gradient accumulators (raster_kernel's housekeeping loop)


def _zero_fill_scene(name):
    if name == "case1":  # many workgroups share the fill
        return scenes.random_triangles(F=400, W=67, H=45, radius_px=9.0, seed=0), 7
    return scenes.random_triangles(F=60, W=1, H=1, C=1, radius_px=2.0, seed=102), 3  # one workgroup fills everything


@pytest.mark.parametrize("which", ["both", "vertices_only", "colors_only"])
@pytest.mark.parametrize("offset", [4, 1], ids=["aligned16", "offset4"])
@pytest.mark.parametrize("name", ["case1", "frame_1x1"])
def test_resolve_zero_fills_the_accumulators(name, offset, which):
    """Accumulators prefilled with 7.0 inside guard elements, 16-B aligned (a view 4 floats in) or at a 4-byte offset
    (a view 1 float in: the scalar fill), each of the two NULL in turn: after the resolve every element is exactly 0
    and the guards still 7.0, and a DIRT_BWD_ACCUMULATE backward into them gives the oracle's gradients."""
    from dirt_amd import _lib
    scene, C2 = _zero_fill_scene(name)
    bg1, v, c1, f = _batched(scene)
    first = _FirstForward(bg1, v, c1, f)
    V = v.shape[1]
    bg2, c2 = _render_inputs(bg1.shape[:3], V, C2, 16)
    want_v, want_c = which != "colors_only", which != "vertices_only"
    bufs, views = [], []
    for n, want in ((V * 4, want_v), (V * C2, want_c)):
        buf = torch.full((n + 8,), 7.0, device="cuda") if want else None
        bufs.append(buf)
        views.append(buf[offset:offset + n] if want else None)
    for vw in views:
        if vw is not None:
            assert (vw.data_ptr() % 16 == 0) == (offset == 4)
    _, ct, px, gb = first.resolve(bg2, c2, views[0], views[1])
    torch.cuda.synchronize()
    for buf, n in zip(bufs, (V * 4, V * C2)):
        if buf is not None:
            h = buf.cpu().numpy()
            assert np.all(h[:offset] == 7.0) and np.all(h[offset + n:] == 7.0), "a guard element was written"
            assert np.all(h[offset:offset + n] == 0.0) and not np.signbit(h[offset:offset + n]).any()
    ref_px, ref_gb, _ = oracle.rasterise_fwd(bg2, v, c2, f)
    np.testing.assert_array_equal(px.cpu().numpy(), ref_px)
    gp = np.random.default_rng(17).standard_normal(bg2.shape).astype(np.float32)
    rgv, rgc, rgbg = oracle.rasterise_bwd(v, c2, f, ref_px, gp, ref_gb)
    gbg, _, _ = first.backward(ct, px, gb, gp, gv=views[0], gc=views[1], flags=_lib.BWD_ACCUMULATE,
                               want=(want_v, want_c))
    np.testing.assert_array_equal(gbg.cpu().numpy(), rgbg)
    if want_v:
        assert_close_grad(views[0].cpu().numpy().reshape(1, V, 4), rgv, "grad_vertices")
    if want_c:
        assert_close_grad(views[1].cpu().numpy().reshape(1, V, C2), rgc, "grad_vertex_colors")
    for buf, n in zip(bufs, (V * 4, V * C2)):
        if buf is not None:
            h = buf.cpu().numpy()
            assert np.all(h[:offset] == 7.0) and np.all(h[offset + n:] == 7.0), "the backward wrote a guard element"
    first.assert_only_read()
