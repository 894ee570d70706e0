"""GPU pin of the forward: the HIP kernels against the exact statement of DESIGN.md 3 (tests/forward_exact.py)
directly -- no oracle call.  The outputs are read through dirt_amd.rasterise_batch_gbuffer (pixels, depth,
barycentrics, face ids: the G-buffer raster variants) and through _rasterise_batched(..., return_gbuffer=True)
(pixels and the g-buffer word: the plain variants); both sets of pixels must be the same bits.  Assertions as
in tests/test_forward_exact.py, at every pixel; the cases are that file's (tests/forward_cases.py), so the 2 %
cap on undecided pixels is a condition already checked on the CPU and asserted again here.

Each forward path at the smallest shape at which it exists: the fused small-scene raster (F = 32) and the
binned one on the same two 40x24 frames (F = 33; partial tiles right and bottom); the binned path with slabs
too small for its bins (the overflow fallback); the occluder-culling raster forced on the deep stacks; clipped
faces, interpenetrating pairs, near / far straddlers, exact ties and the flat-depth known answers at 33x17 and
64x48; the channel classes 1, 3, 7 and 5 (generic), binned (F = 60) and fused (F = 32); 1x17 and 17x1 frames.

Measured on an MI355X, worst |kernel - exact| / (2^-24 sum |terms|) over these cases: depth 1.73 (k = 8,
clipped_64x48), barycentrics 4.79 (k = 13) and colours 4.80 (k = 16) on near_far_outside_64x48 -- the CPU table's
figures, as the kernels are bit-identical to the oracle; undecided at most 1.66 % (deep stacks).  30 tests, each
under a second.
"""
import numpy as np
import pytest
import torch

import forward_cases
import scenes

pytestmark = pytest.mark.gpu


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_and_check(name, bin_capacity=0):
    """Both raster variants of the public path on a case, every assertion of the pin on each."""
    import dirt_amd
    from dirt_amd import rasterise_ops
    (bg, v, c, f), _ = forward_cases.case(name)
    B, H, W, C = bg.shape
    t = tuple(_gpu(a) for a in (bg, v, c, f))
    px, gb = rasterise_ops._rasterise_batched(*t, None, H, W, C, 0, bin_capacity, return_gbuffer=True)
    px, gb = px.cpu().numpy(), gb.cpu().numpy()
    if bin_capacity:
        outs = rasterise_ops._rasterise_batched(*t, None, H, W, C, 0, bin_capacity, want_gbuf=True)
        g = rasterise_ops.GBuffer(outs[0], *outs[2:])
        assert np.array_equal(outs[1].cpu().numpy(), gb)
    else:
        g = dirt_amd.rasterise_batch_gbuffer(*t)
    gpx, depth, bary, face = (x.cpu().numpy() for x in g)
    assert np.array_equal(gpx.view(np.uint32), px.view(np.uint32))
    forward_cases.check(name, px, gbuffer=gb, label=" (plain raster)")
    return forward_cases.check(name, gpx, gbuffer=gb, depth=depth, barycentrics=bary, face_ids=face,
                               label=" (G-buffer raster)")


@pytest.mark.parametrize("name", ["small_F32", "small_F33"])
def test_fused_and_binned_paths_on_the_same_frames(name):
    """F = 32 takes the fused small-scene raster, the same frames with one more face the setup + binned one."""
    run_and_check(name)


def test_bin_overflow_fallback():
    """300 faces with 64 bin entries in all: every slab overflows and the raster filters the records itself."""
    run_and_check("random_affine", bin_capacity=64)


@pytest.mark.parametrize("name", ["deep_affine", "deep_perspective"])
def test_deep_cull_raster(name):
    """The occluder-culling raster (DIRT_FWD_DEEP_CULL forced, as test_deep_cull_flag_bit_exact forces it) on the
    deep stacks: about 90 records per pixel, exact ties and near ties.  A session returns pixels and the g-buffer
    word; the default rasters on the same case give the G-buffer outputs."""
    from dirt_amd.session import RasteriseSession
    (bg, v, c, f), _ = forward_cases.case(name)
    sess = RasteriseSession(*bg.shape, v.shape[1], f.shape[1], device="cuda", deep_cull=True)
    sess.forward(*(_gpu(a) for a in (bg, v, c, f)))
    forward_cases.check(name, sess.pixels.cpu().numpy(), gbuffer=sess.gbuffer.cpu().numpy(), label=" (deep cull)")
    run_and_check(name)


@pytest.mark.parametrize("size", forward_cases.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ["clipped", "interpenetrating_affine", "interpenetrating_perspective",
                                    "near_far_inside", "near_far_outside"])
def test_depth_and_clipping_cases(family, size):
    run_and_check("%s_%dx%d" % ((family,) + size))


@pytest.mark.parametrize("size", forward_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_exact_ties(size):
    """Duplicates of one ordered vertex triple: decided by the statement, so the word check of the pin already
    requires the original; no duplicate may be visible anywhere."""
    import dirt_amd
    name = "exact_ties_%dx%d" % size
    run_and_check(name)
    _, pairs = scenes.exact_tie_scene(size[0] % 2, W=size[0], H=size[1])
    (bg, v, c, f), _ = forward_cases.case(name)
    face = dirt_amd.rasterise_batch_gbuffer(*(_gpu(a) for a in (bg, v, c, f))).face_ids.cpu().numpy()
    assert not np.isin(face, [d for _, d in pairs]).any()
    assert np.isin(face, [o for o, _ in pairs]).any()


@pytest.mark.parametrize("size", forward_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_flat_depth_known_answers(size):
    """Constant-zw quads (tests/test_forward_exact.py::test_flat_depth_known_answers): zw = 0, 0.25, 0.5 and
    1 - 2^-23 give d = 0, 2^22, 2^23 and 2^24 - 2 exactly; 1 - 2^-24 and 1.0 are invisible."""
    import dirt_amd
    W, H = size
    name = "flat_depth_%dx%d" % size
    run_and_check(name)
    _, spans = scenes.flat_depth_scene(W=W, H=H)
    (bg, v, c, f), _ = forward_cases.case(name)
    g = dirt_amd.rasterise_batch_gbuffer(*(_gpu(a) for a in (bg, v, c, f)))
    px, depth, face = g.pixels.cpu().numpy()[0], g.depth.cpu().numpy()[0], g.face_ids.cpu().numpy()[0]
    M = (1 << 24) - 1
    rows = slice(H // 8 + 1, H - H // 8 - 1)
    for q, ((x0, x1), d) in enumerate(zip(spans, (0, 1 << 22, 1 << 23, M - 1, None, None))):
        if d is None:
            assert (face[rows, x0:x1] == -1).all() and (depth[rows, x0:x1] == np.float32(1.0)).all(), q
            assert np.array_equal(px[rows, x0:x1], bg[0][rows, x0:x1]), q
        else:
            assert np.isin(face[rows, x0:x1], (2 * q, 2 * q + 1)).all(), q
            assert (depth[rows, x0:x1] == np.float32(d) / np.float32(M)).all(), q


@pytest.mark.parametrize("name", ["channels_%d" % C for C in (1, 3, 7, 5)] +
                         ["channels_fused_%d" % C for C in (1, 3, 7, 5)],
                         ids=["1", "3", "7", "5", "fused_1", "fused_3", "fused_7", "fused_5"])
def test_channel_classes(name):
    """The channel specialisations 1, 3, 7 and the generic one (5) at 40x24: 60 overlapping perspective faces
    (setup + binned raster), and 32 (the fused small-scene raster), each plain and with the G-buffer outputs."""
    run_and_check(name)


@pytest.mark.parametrize("name", ["line_1x17", "line_17x1"])
def test_one_pixel_wide_frames(name):
    run_and_check(name)


def test_fuzz_seed_37851():
    """The two-frame, five-channel fuzz case with clipped faces and coplanar overlaps."""
    run_and_check("fuzz_37851")
