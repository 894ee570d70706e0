"""The scene table of the forward pin (tests/forward_exact.py): named batched scenes of at most 64x48 pixels,
built once per process with their statements, shared by tests/test_forward_exact.py (the oracle against the
statement, every case) and tests/test_gpu_forward_exact.py (the HIP kernels against it, the cases each forward
path needs).  TEST INFRASTRUCTURE ONLY.

CAP: a condition on the inputs, not a measurement -- at most 2 % of a case's covered pixels may be undecided by
the statement alone, or the case pins too little.  The adversarial fuzz scenes (coplanar faces with different
vertex triples, which no bound can order) are membership-only: no cap, the share is printed."""
import functools

import forward_exact
import scenes

CAP = 0.02
SIZES = ((64, 48), (33, 17))


def _batched(sc):
    return tuple(a[None] for a in sc) if sc[0].ndim == 3 else tuple(sc)


def _small(F):
    """Two 40x24 frames (partial tiles at the right and the bottom) of the same 33 overlapping faces, cut to F."""
    bg, v, c, f = scenes.batch_of(scenes.random_triangles, 2, F=33, W=40, H=24, radius_px=12.0, seed=21)
    return bg, v[:, :3 * F], c[:, :3 * F], f[:, :F]


def _clipped(W, H):
    return scenes.clipping_scene(W=W, H=H)


CASES = {
    "random_affine": lambda: scenes.random_triangles(F=300, W=64, H=48, radius_px=10.0, seed=1),
    "random_perspective": lambda: scenes.random_triangles(F=300, W=64, H=48, radius_px=10.0, seed=2, perspective=True),
    "fuzz_37851": lambda: scenes.fuzz_case(37851),
    "deep_affine": lambda: scenes.deep_scene(False, W=64, H=48),
    "deep_perspective": lambda: scenes.deep_scene(True, W=64, H=48),
    "small_F32": lambda: _small(32),
    "small_F33": lambda: _small(33),
    "line_1x17": lambda: scenes.random_triangles(F=24, W=1, H=17, radius_px=6.0, seed=5),
    "line_17x1": lambda: scenes.random_triangles(F=24, W=17, H=1, radius_px=6.0, seed=6, perspective=True),
}
for _s in range(5):
    CASES["clipped_sliver_%d" % _s] = functools.partial(scenes.clipped_sliver_scene, _s)
for _C in (1, 3, 7, 5):
    CASES["channels_%d" % _C] = functools.partial(scenes.random_triangles, F=60, W=40, H=24, C=_C, radius_px=10.0,
                                                  seed=30 + _C, perspective=True)
    # at most kFusedMaxF = 32 faces: the fused small-scene forward (no setup launch, no bins) of the channel class
    CASES["channels_fused_%d" % _C] = functools.partial(scenes.random_triangles, F=32, W=40, H=24, C=_C,
                                                        radius_px=10.0, seed=40 + _C, perspective=True)
for _W, _H in SIZES:
    _t = "_%dx%d" % (_W, _H)
    CASES["clipped" + _t] = functools.partial(_clipped, _W, _H)
    CASES["interpenetrating_affine" + _t] = functools.partial(scenes.interpenetrating_scene, 0, W=_W, H=_H)
    CASES["interpenetrating_perspective" + _t] = functools.partial(scenes.interpenetrating_scene, 1, W=_W, H=_H,
                                                                   perspective=True)
    CASES["near_far_inside" + _t] = functools.partial(scenes.near_far_scene, 0, W=_W, H=_H)
    CASES["near_far_outside" + _t] = functools.partial(scenes.near_far_scene, 0, W=_W, H=_H, outside=True)
    CASES["exact_ties" + _t] = lambda W=_W, H=_H: scenes.exact_tie_scene(W % 2, W=W, H=H)[0]
    CASES["flat_depth" + _t] = lambda W=_W, H=_H: scenes.flat_depth_scene(W=W, H=H)[0]
MEMBERSHIP_ONLY = {}
for _s in range(4):
    MEMBERSHIP_ONLY["adversarial_%d" % _s] = functools.partial(scenes.adversarial_scene, _s)


@functools.lru_cache(maxsize=None)
def case(name):
    """(background, vertices, colours, faces) of a case, batched, and the statement of every frame."""
    bg, v, c, f = _batched((CASES.get(name) or MEMBERSHIP_ONLY[name])())
    B, H, W, _ = bg.shape
    return (bg, v, c, f), [forward_exact.Frame(v[b], f[b], W, H) for b in range(B)]


def check(name, pixels, gbuffer=None, depth=None, barycentrics=None, face_ids=None, label=""):
    """forward_exact.check_frame on every frame of a case; prints the worst ratios and the undecided share and
    asserts the cap (a condition on the case's inputs).  Returns the figures of the whole case."""
    (bg, v, c, f), frames = case(name)
    tot = {"depth": 0.0, "barycentrics": 0.0, "colours": 0.0, "covered": 0, "undecided": 0}
    for b, fr in enumerate(frames):
        r = forward_exact.check_frame(fr, bg[b], c[b], pixels[b], None if gbuffer is None else gbuffer[b],
                                      None if depth is None else depth[b],
                                      None if barycentrics is None else barycentrics[b],
                                      None if face_ids is None else face_ids[b])
        for k in ("depth", "barycentrics", "colours"):
            tot[k] = max(tot[k], r[k])
        tot["covered"] += r["covered"]
        tot["undecided"] += r["undecided"]
    tot["share"] = tot["undecided"] / max(tot["covered"], 1)
    print("%s%s: worst error / (2^-24 sum|terms|): depth %.2f (k = %d), barycentrics %.2f (k = %d), colours %.2f "
          "(k = %d); undecided %d of %d covered pixels = %.2f %%" % (
              name, label, tot["depth"], forward_exact.K_DEPTH, tot["barycentrics"], forward_exact.K_BARY,
              tot["colours"], forward_exact.K_COLOUR, tot["undecided"], tot["covered"], 100.0 * tot["share"]))
    if name in CASES:
        assert tot["covered"] > 0 and tot["share"] <= CAP, "%s: %.2f %% of the covered pixels are undecided" % (
            name, 100.0 * tot["share"])
    return tot
