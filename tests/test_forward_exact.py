"""CPU pin of the forward: the oracle (oracle/dirt_oracle.c) against the exact statement of DESIGN.md 3
(tests/forward_exact.py) -- depth (R4), clipping (R5), the visible record, colours (R6) and the depth /
barycentrics / face_ids G-buffer outputs, at every pixel of every case of tests/forward_cases.py:
  * the reported face is a possible winner; background only where no record is certainly in range;
  * on decided pixels the g-buffer word is the statement's (record index, bit 30 for a clipped face);
  * depth is d / (2^24 - 1) for a d inside the record's interval; barycentrics and pixels within their bounds;
  * uncovered pixels: the background bit for bit, depth 1.0, barycentrics 0;
  * at most 2 % of a case's covered pixels undecided (a condition on the inputs; asserted per case).

Measured on this table, worst |oracle - exact| / (2^-24 sum |terms|) against the derived constants of
forward_exact.py: depth 1.73 (K_DEPTH = 8; a lower bound of the error, read from d alone; clipped_64x48),
barycentrics 4.79 (K_BARY = 13) and colours 4.80 (K_COLOUR = 16), both on near_far_outside_64x48.  Undecided:
0 % on the random, interpenetrating, near / far, tie and flat cases, 0.07 % clipped_64x48, at most 0.36 % on the
clipped slivers, 0.93 % fuzz seed 37851, 1.66 % on the deep stacks (their 80 near-tie copies); 0 to 3.1 % on the
adversarial seeds (membership only).  Every test prints its own figures.

What a wrong reading costs (checked on edited copies of the oracle): the tie-break flipped to the highest face
fails, on decided pixels, the cases deep_affine, deep_perspective, exact_ties_*, fuzz_37851, the four
adversarial seeds and test_exact_ties_resolve_to_the_lowest_face; `d < 2^24 - 1` dropped fails the flat_depth_*
cases and test_flat_depth_known_answers; two sub-triangle record numbers swapped in the statement fail the
clipped cases (test_swapped_record_numbers_fail_the_clipped_cases).
"""
import functools

import numpy as np
import pytest

import forward_cases
import forward_exact
import scenes
from oracle import oracle

M = forward_exact.DEPTH_MAX


@functools.lru_cache(maxsize=None)
def oracle_outputs(name):
    (bg, v, c, f), _ = forward_cases.case(name)
    px, gb, depth, bary, face, _ = oracle.rasterise_fwd_gbuffer(bg, v, c, f)
    px2, gb2, _ = oracle.rasterise_fwd(bg, v, c, f)  # the plain forward writes the same pixels and words
    assert np.array_equal(px.view(np.uint32), px2.view(np.uint32)) and np.array_equal(gb, gb2)
    return px, gb, depth, bary, face


@pytest.mark.parametrize("name", sorted(forward_cases.CASES))
def test_oracle_against_the_exact_statement(name):
    px, gb, depth, bary, face = oracle_outputs(name)
    forward_cases.check(name, px, gb, depth, bary, face)


@pytest.mark.parametrize("name", sorted(forward_cases.MEMBERSHIP_ONLY))
def test_oracle_membership_on_adversarial_scenes(name):
    """Coplanar faces with different vertex triples: the statement cannot order them (0 to 3.1 % of the covered
    pixels undecided on these seeds), so no cap -- every other assertion holds at every pixel."""
    px, gb, depth, bary, face = oracle_outputs(name)
    forward_cases.check(name, px, gb, depth, bary, face)


@pytest.mark.parametrize("size", forward_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_exact_ties_resolve_to_the_lowest_face(size):
    """Duplicates of one ordered (X, Y, zw) triple at face-index distances 1 .. 40: wherever the statement sees
    the original as a possible winner the pixel is decided, the oracle shows the original, never the duplicate."""
    W, H = size
    name = "exact_ties_%dx%d" % size
    _, pairs = scenes.exact_tie_scene(W % 2, W=W, H=H)
    _, (fr,) = forward_cases.case(name)
    face = oracle_outputs(name)[4][0]
    dups = {d: o for o, d in pairs}
    assert not np.isin(face, list(dups)).any()
    shown = 0
    for j in range(H):
        for i in range(W):
            win = fr.winners[j][i]
            assert not any(int(fr.face[a]) in dups for a in win), (i, j)
            if len(win) == 1 and int(fr.face[win[0]]) in dups.values():
                assert face[H - 1 - j, i] == fr.face[win[0]], (i, j)
                shown += 1
    assert shown > 0 and len({d - o for o, d in pairs}) >= 4
    print("%s: %d decided pixels show an original in front of its duplicate" % (name, shown))


@pytest.mark.parametrize("size", forward_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_flat_depth_known_answers(size):
    """Constant-zw quads: d is the exact quantisation -- 0 -> 0, 0.25 -> 2^22, 0.5 -> 2^23, 1 - 2^-23 -> 2^24 - 2
    (the largest visible depth); 1 - 2^-24 rounds to 2^24 - 1 in R4's float32 fma and is invisible like 1.0."""
    W, H = size
    name = "flat_depth_%dx%d" % size
    _, spans = scenes.flat_depth_scene(W=W, H=H)
    (bg, v, c, f), (fr,) = forward_cases.case(name)
    px, gb, depth, bary, face = (a[0] for a in oracle_outputs(name))
    expect = (0, 1 << 22, 1 << 23, M - 1, None, None)
    assert [forward_exact.quantise(z) for z in scenes.FLAT_DEPTHS] == [0, 1 << 22, 1 << 23, M - 1, M, M + 1]
    rows = slice(H // 8 + 1, H - H // 8 - 1)  # the quads span y in [-0.75, 0.75]
    for q, ((x0, x1), d) in enumerate(zip(spans, expect)):
        if d is None:
            assert (face[rows, x0:x1] == -1).all() and (depth[rows, x0:x1] == np.float32(1.0)).all(), q
            assert np.array_equal(px[rows, x0:x1], bg[0][rows, x0:x1]), q
        else:
            assert np.isin(face[rows, x0:x1], (2 * q, 2 * q + 1)).all(), q
            assert (depth[rows, x0:x1] == np.float32(d) / np.float32(M)).all(), q


def test_covers_grid_is_covers():
    """The vectorised coverage the statement uses is `Tri.covers` pixel by pixel (clipped records included)."""
    _, (fr,) = forward_cases.case("clipped_33x17")
    n = 0
    for ri, (f, s, t, clipped) in fr.rec_tri.items():
        inside, _ = t.covers_grid(0, fr.W - 1, 0, fr.H - 1)
        for j in range(fr.H):
            for i in range(fr.W):
                assert inside[j, i] == t.covers(i, j)
        n += clipped
    assert n > 0


def test_swapped_record_numbers_fail_the_clipped_cases():
    """The statement's record numbering is load-bearing: with sub-triangles 1 and 2 of every clipped face
    swapped, the oracle's g-buffer word no longer matches on the clipped cases."""
    def swapped(F, f, s):
        return forward_exact.record_index(F, f, {1: 2, 2: 1}.get(s, s))
    for name in ("clipped_64x48", "near_far_outside_64x48", "clipped_sliver_1"):
        (bg, v, c, f), _ = forward_cases.case(name)
        px, gb, depth, bary, face = oracle_outputs(name)
        fr = forward_exact.Frame(v[0], f[0], bg.shape[2], bg.shape[1], record=swapped)
        with pytest.raises(AssertionError):
            forward_exact.check_frame(fr, bg[0], c[0], px[0], gb[0], depth[0], bary[0], face[0])
