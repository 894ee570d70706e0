"""CPU pin of the backward: the oracle (oracle/dirt_oracle.c) against an independent float64 restatement of the
specification (tests/backward_f64.py), DESIGN.md 4 / SURVEY Appendix B.

The reference registers no gradient, so nothing reference-held pins the backward; this is the
second statement of it, written from the spec in float64 (normalised perspective-correct barycentrics, the
clip w of the pair midpoint, the chain rule through the window transform) -- the oracle evaluates the same
quantities in float32 through the cancellation-free identity lambda_k / Wm = a_k / (2D).  Contract:
  * grad_background identical;
  * grad_vertices and grad_vertex_colors within 1e-6 of the gradient's scale (max |float64|), on every golden
    scene, the fuzz scene that exposed the normalised form's cancellation (seed 37851, a 1811-unit sliver) and
    50 clipped-sliver scenes (guard-band and near-plane clipping; the old normalised clipped weight failed 9
    of them, up to 8.6e-6: profiles/r04/f64_pin.txt).
"""
import glob
import os

import numpy as np
import pytest

import backward_cases
import backward_f64
import scenes
from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIN = 1e-6


def check_pin(bg, v, c, f, seed):
    gp = np.random.default_rng(seed).standard_normal(bg.shape).astype(np.float32)
    px, gb, _ = oracle.rasterise_fwd(bg, v, c, f)
    gv64, gc64, gbg64 = backward_f64.backward_batch(v, f, px, gp, gb)
    gv, gc, gbg = oracle.rasterise_bwd(v, c, f, px, gp, gb)
    np.testing.assert_array_equal(gbg, gbg64.astype(np.float32))
    ev, ec = backward_f64.max_rel_err(gv, gv64), backward_f64.max_rel_err(gc, gc64)
    assert ev <= PIN, "grad_vertices: %.3g of the scale vs float64" % ev
    assert ec <= PIN, "grad_vertex_colors: %.3g of the scale vs float64" % ec
    return gb


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))), ids=os.path.basename)
def test_f64_pin_golden_scenes(path):
    z = np.load(path)
    gp = z["grad_pixels"]
    gv64, gc64, gbg64 = backward_f64.backward_batch(z["vertices"], z["faces"], z["pixels"], gp, z["gbuffer"])
    np.testing.assert_array_equal(z["grad_background"], gbg64.astype(np.float32))
    # the committed fixture (oracle output) and a fresh oracle run
    gv, gc, _ = oracle.rasterise_bwd(z["vertices"], z["vertex_colors"], z["faces"], z["pixels"], gp, z["gbuffer"])
    for a, b, name in ((z["grad_vertices"], gv64, "fixture grad_vertices"), (z["grad_vertex_colors"], gc64,
                       "fixture grad_vertex_colors"), (gv, gv64, "grad_vertices"), (gc, gc64, "grad_vertex_colors")):
        e = backward_f64.max_rel_err(a, b)
        assert e <= PIN, "%s: %.3g of the scale vs float64" % (name, e)


def test_f64_pin_fuzz_seed_37851():
    """The round-3 fuzz campaign's sliver, rebuilt from its seed: batch of two 64x48 frames, 5
    channels, with clipped faces."""
    bg, v, c, f = scenes.fuzz_case(37851)
    gb = check_pin(bg, v, c, f, 37851)
    assert ((gb >= 0) & ((gb & (1 << 30)) != 0)).any()  # clipped faces are visible


def test_f64_pin_sub_vertex_beyond_guard_band():
    """Fuzz seed 167059 (batch of two 33x17 frames, 5 channels): clipping faces 71 and 115 of frame 0 leaves a
    sub-vertex at x/w = -4.7e6 (w = 7e-12), far outside the guard band; R5's sub-vertex clamp (twice the band)
    keeps its snapped coordinates, and so every edge coefficient, inside the integer ranges both sides assume."""
    bg, v, c, f = scenes.fuzz_case(167059)
    B, H, W, C = bg.shape
    for fi in (71, 115):
        tris, clipped = backward_f64.setup_face(v[0], f[0][fi], v.shape[1], W, H)
        assert clipped and len(tris) == 3
        assert all(abs(x) < 2 ** 25 for t in tris if t is not None for x in t.A + t.B)
    check_pin(bg, v, c, f, 167059)


def test_f64_pin_clip_vertex_cap():
    """scenes.near_w0_scene seed 41533: a face whose clipped polygon exceeds 8 vertices (rounding near w = 0);
    R5's vertex cap culls it in the oracle and in the float64 statement alike."""
    bg, v, c, f = (a[None] for a in scenes.near_w0_scene(41533, W=33, H=17, C=1))
    before = backward_f64.CAP_CULLS[0]
    for fi in range(f.shape[1]):
        backward_f64.setup_face(v[0], f[0][fi], v.shape[1], 33, 17)
    assert backward_f64.CAP_CULLS[0] > before
    check_pin(bg, v, c, f, 41533)


@pytest.mark.parametrize("block", range(5))
def test_f64_pin_clipped_slivers(block):
    """50 scenes of guard-band and near-plane clipped slivers (10 per case)."""
    for seed in range(10 * block, 10 * block + 10):
        bg, v, c, f = (a[None] for a in scenes.clipped_sliver_scene(seed))
        check_pin(bg, v, c, f, seed)


# ---- the per-element contract (tests/backward_cases.py: derivation, case table) -----------------------------------
def _oracle_within_bound(ref, label):
    bg, v, c, f = ref.inputs
    gv, gc, gbg = oracle.rasterise_bwd(v, c, f, ref.px, ref.gp, ref.gb)
    backward_cases.check_background(gbg, ref)
    ratios = backward_cases.check_bound(gv, gc, ref, in_double=True)
    print("\n" + backward_cases.fmt(label, ratios))
    return gv, gc


@pytest.mark.parametrize("name", [c.name for c in backward_cases.CASES])
def test_oracle_within_the_derived_bound(name):
    """The oracle (float32 terms summed in double: k u S plus the final cast's half unit) on the whole table, every
    case's condition on its content asserted first."""
    _oracle_within_bound(backward_cases.reference(name), name)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))), ids=os.path.basename)
def test_oracle_and_fixtures_within_the_derived_bound(path):
    z = np.load(path)
    ref = backward_cases.Reference((z["background"], z["vertices"], z["vertex_colors"], z["faces"]), 0,
                                   forward=(z["pixels"], z["gbuffer"]), grad_pixels=z["grad_pixels"])
    _oracle_within_bound(ref, os.path.basename(path))
    backward_cases.check_background(z["grad_background"], ref)
    print(backward_cases.fmt("fixture", backward_cases.check_bound(z["grad_vertices"], z["grad_vertex_colors"], ref,
                                                                   in_double=True)))


def test_with_bounds_returns_the_same_values():
    ref = backward_cases.reference("clipped_sliver_0")
    bg, v, c, f = ref.inputs
    for a, b in zip(backward_f64.backward_batch(v, f, ref.px, ref.gp, ref.gb), (ref.gv, ref.gc, ref.gbg)):
        np.testing.assert_array_equal(a, b)


def _apply(gv, gc, frame, edits):
    """Copies of the (float32) gradients with `edits` -- (tensor, vertex, column, delta) -- added in frame `frame`."""
    gv, gc = gv.astype(np.float64), gc.astype(np.float64)
    for tensor, v, col, delta in edits:
        (gv if tensor == "v" else gc)[frame, v, col] += delta
    return gv.astype(np.float32), gc.astype(np.float32)


def _pair_edits(t, sign):
    """One pair term of the statement, `sign` times, as edits of its two elements."""
    return [("v", t["vertex"], t["axis"], sign * t["g"]), ("v", t["vertex"], 3, -sign * t["g"] * t["ndc"])]


def _mutations(ref, frame):
    """Wrong gradients built from the statement's own terms: name -> list of candidate edit lists."""
    terms = ref.bounds[frame].terms
    W = ref.gb.shape[2]
    pairs = [t for t in terms if t["kind"] == "pair" and t["g"] != 0.0]
    by_pair = {}
    for t in pairs:
        by_pair.setdefault((t["pixel"], t["axis"]), []).append(t)
    split = []
    for ts in by_pair.values():
        if ts[0]["omega"] == 0.5 and len({t["record"] for t in ts}) == 2:
            first = ts[0]["record"]  # 0.5 / 0.5 -> 1 / 0: the first owner takes the other's half
            split.append(sum((_pair_edits(t, 1.0 if t["record"] == first else -1.0) for t in ts), []))
    return {
        "one pair term removed": [_pair_edits(t, -1.0) for t in pairs],
        "one pair term added twice": [_pair_edits(t, 1.0) for t in pairs],
        # dL/dw of an x pair with the next pair's x_ndc = x_ndc + 2 / W
        "w component with the neighbouring pair's x_ndc": [[("v", t["vertex"], 3, -t["g"] * 2.0 / W)]
                                                           for t in pairs if t["axis"] == 0],
        "0.5 / 0.5 split turned into 1 / 0": split,
        "colour term of one covered pixel dropped": [[("c", t["vertex"], ch, -t["g"][ch]) for ch in range(ref.C)]
                                                     for t in terms if t["kind"] == "colour" and np.any(t["g"] != 0.0)],
    }


VERTEX_MUTANTS = ("one pair term removed", "one pair term added twice", "w component with the neighbouring pair's x_ndc",
                  "0.5 / 0.5 split turned into 1 / 0")
COLOUR_MUTANTS = ("colour term of one covered pixel dropped",)


@pytest.mark.parametrize("name,labels", [("fuzz_167059", VERTEX_MUTANTS), ("fuzz_37851", VERTEX_MUTANTS),
                                         ("bright_half", COLOUR_MUTANTS)])
def test_wrong_terms_on_small_elements_fail_the_bound_and_pass_the_scale_relative_contract(name, labels):
    """The gap the per-element contract closes.  The oracle's output is corrupted on elements below 1e-4 of the
    gradient's scale by one wrong term of the float64 statement (its effect on that element); every such mutant fails
    check_bound, and passes
    tests/test_gpu_parity.py::assert_close_grad -- the ordinary and even the strict pair, against the float64
    values -- because the scale of the tensor, set by the scene's sliver (the colours': by the vertices of a face that
    fills the frame), hides it."""
    from test_gpu_parity import assert_close_grad
    if name == "bright_half":
        # the colour gradients' scale is a few tens on every table case (no term below 1e-5 of it); a cotangent 4096
        # times larger on the left half of the frame -- a loss that weighs one region -- sets it for the right half
        case = backward_cases.BY_NAME["frame_64x48"]
        gp = np.random.default_rng(5).standard_normal((1, 48, 64, 3)).astype(np.float32)
        gp[:, :, :32] *= np.float32(4096.0)
        ref = backward_cases.Reference(case.build(), 5, True, grad_pixels=gp)
    else:
        ref = backward_cases.reference(name, True)
    bg, v, c, f = ref.inputs
    gv, gc, _ = oracle.rasterise_bwd(v, c, f, ref.px, ref.gp, ref.gb)
    bound = {"v": ref.bound_vertices(True), "c": ref.bound_colours(True)}
    want = {"v": ref.gv, "c": ref.gc}
    scale = {k: np.abs(a).max() for k, a in want.items()}
    frame = 0
    mutations = _mutations(ref, frame)
    assert set(mutations) == set(VERTEX_MUTANTS + COLOUR_MUTANTS)
    for label in labels:
        candidates, chosen = mutations[label], None
        for edits in candidates:
            tot = {}  # (an element the edits touch twice -- a vertex of both owners -- gets their sum)
            for tensor, vtx, col, d in edits:
                tot[(tensor, vtx, col)] = tot.get((tensor, vtx, col), 0.0) + d
            for (t, vx, col), d in tot.items():
                # a small element, on which the wrong term is far outside the bound and far inside 1e-6 of the scale
                if abs(want[t][frame, vx, col]) < 1e-4 * scale[t] and \
                        2.0 * bound[t][frame, vx, col] < abs(d) <= 0.4e-6 * scale[t]:
                    chosen = [(t, vx, col, d)]
                    break
            if chosen:
                break
        assert chosen is not None, "no candidate for: " + label
        mv, mc = _apply(gv, gc, frame, chosen)
        with pytest.raises(AssertionError, match="over the bound"):
            backward_cases.check_bound(mv, mc, ref, in_double=True)
        for strict in (False, True):
            assert_close_grad(mv, ref.gv, "grad_vertices", strict)
            assert_close_grad(mc, ref.gc, "grad_vertex_colors", strict)
        t, vx, col, d = chosen[0]
        print("%s / %s: element %s[%d, %d] = %.3g (%.1e of the scale), wrong by %.3g = %.0f bounds: fails the bound, "
              "passes the scale-relative contract" % (name, label, t, vx, col, want[t][frame, vx, col],
                                                      abs(want[t][frame, vx, col]) / scale[t], d,
                                                      abs(d) / bound[t][frame, vx, col]))


def test_f64_restatement_readme_square_kats():
    """The float64 statement on its own satisfies the README square's translation KATs (README.md:41):
    d(sum pixels)/d centre_x = 0 and d(sum x pixels)/d centre_x = area (256 px, 16x16 square, C = 1)."""
    bg, v, c, f = scenes.readme_square()
    px, gb, _ = oracle.rasterise_fwd(bg[None], v[None], c[None], f[None])
    H, W = bg.shape[:2]
    ones = np.ones((1, H, W, 1), np.float32)
    xs = np.broadcast_to(np.arange(W, dtype=np.float32)[None, None, :, None], (1, H, W, 1)).copy()
    for g, expect in ((ones, 0.0), (xs, 256.0)):
        gv, _, _ = backward_f64.backward_batch(v[None], f[None], px, g, gb)
        # centre_x moves every vertex's clip x by the same amount: d/dcentre_x in window px = sum_v dL/dx_v * (2/W)
        d = float(gv[0, :, 0].sum()) * 2.0 / W
        assert abs(d - expect) <= 1e-9 + 0.05 * abs(expect), (d, expect)
