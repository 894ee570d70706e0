"""CPU pin of the rasteriser at full frame size: the oracle (oracle/dirt_oracle.c) against windows of the two
statements on the frames of tests/large_frame_cases.py (4096x4096 to 8192x8192), and the windowing itself against
the dense statements on three small cases.

  * Windowing (forward_exact.Frame / check_frame and backward_f64.backward with `window`): the full-frame window
    is the dense statement, a proper sub-window is the dense statement restricted to it, and the backward of a
    cotangent supported on a sub-window is bit-identical dense and windowed, Bounds included.
  * Forward, every (case, window): pixels, g-buffer word, depth, barycentrics and face ids of the oracle's whole-frame
    outputs under forward_exact.check_frame's assertions (K_DEPTH, K_BARY, K_COLOUR), at most 2 % undecided.
  * Backward, every (case, window): a cotangent supported on the window, the oracle's gradient under the
    per-element bound of tests/backward_cases.py (sums in double), exactly zero where the statement has no term,
    and grad_background = the cotangent where the g-buffer is -1, else 0, over the whole frame.
The figures each test prints are collected in DESIGN.md 5.
"""
import numpy as np
import pytest

import backward_cases as bc
import backward_f64
import forward_cases
import forward_exact
import large_frame_cases as lf
from oracle import oracle

SMALL = ["random_perspective", "clipped_64x48", "fuzz_37851"]
PER_PAIR = ("pix", "rec", "face", "key", "z", "S", "d_lo", "d_hi", "certain", "possible", "flat", "winner")


def _winner_records(fr, i, j):
    i0, _, j0, _ = fr.window
    return sorted(int(fr.rec[a]) for a in fr.winners[j - j0][i - i0])


def _sub_windows(W, H):
    return [(5, 20, 7, 30), (W - 17, W - 1, 0, 15), (0, 0, H - 1, H - 1), (16, 31, H - 9, H - 1)]


@pytest.mark.parametrize("name", SMALL)
def test_full_window_is_the_dense_forward_statement(name):
    (bg, v, c, f), frames = forward_cases.case(name)
    H, W = bg.shape[1:3]
    for b, dense in enumerate(frames):
        fr = forward_exact.Frame(v[b], f[b], W, H, window=(0, W - 1, 0, H - 1))
        for k in PER_PAIR + ("triple", "any_certain", "covered"):
            assert np.array_equal(getattr(fr, k), getattr(dense, k), equal_nan=k in ("z", "S")), k
        assert fr.winners == dense.winners and fr.n == dense.n


@pytest.mark.parametrize("name", SMALL)
def test_sub_window_is_the_dense_forward_statement_restricted(name):
    (bg, v, c, f), frames = forward_cases.case(name)
    H, W = bg.shape[1:3]
    px, gb, depth, bary, face, _ = oracle.rasterise_fwd_gbuffer(bg, v, c, f)
    for b, dense in enumerate(frames):
        for win in _sub_windows(W, H):
            i0, i1, j0, j1 = win
            fr = forward_exact.Frame(v[b], f[b], W, H, window=win)
            di, dj = dense.pix % W, dense.pix // W
            keep = (di >= i0) & (di <= i1) & (dj >= j0) & (dj <= j1)
            assert np.array_equal(fr.pix, (dj[keep] - j0) * fr.ww + (di[keep] - i0))
            for k in PER_PAIR[1:]:
                assert np.array_equal(getattr(fr, k), getattr(dense, k)[keep], equal_nan=k in ("z", "S")), k
            assert np.array_equal(fr.any_certain, dense.any_certain[j0:j1 + 1, i0:i1 + 1])
            assert np.array_equal(fr.covered, dense.covered[j0:j1 + 1, i0:i1 + 1])
            for j in range(j0, j1 + 1):
                for i in range(i0, i1 + 1):
                    assert _winner_records(fr, i, j) == _winner_records(dense, i, j)
            # the values and bounds of a pair are those of the same pair of the dense statement
            for a, d in list(zip(np.nonzero(fr.winner)[0], np.nonzero(dense.winner & keep)[0]))[::7]:
                for x, y in zip(fr.values(a, c[b]), dense.values(d, c[b])):
                    assert np.array_equal(x, y)
            forward_exact.check_frame(fr, bg[b], c[b], px[b], gb[b], depth[b], bary[b], face[b])


@pytest.mark.parametrize("name", SMALL)
def test_windowed_backward_is_the_dense_one(name):
    """grad_pixels zeroed outside a window: gradients and every Bounds field bit-identical, on every frame, for the
    full-frame window (a dense cotangent), an inner sub-window, one that touches column 0 and row 0 (the halo is cut
    at the frame's border) and one that touches the last column and the last row."""
    (bg, v, c, f), _ = forward_cases.case(name)
    B, H, W, C = bg.shape
    px, gb, _ = oracle.rasterise_fwd(bg, v, c, f)
    windows = [(0, W - 1, 0, H - 1), (9, 40, 11, 34), (0, 14, 0, 9), (W - 20, W - 1, H - 13, H - 1)]
    for b, win in [(b, win) for b in range(B) for win in windows]:
        i0, i1, j0, j1 = win
        gp = np.zeros((H, W, C), np.float32)
        gp[H - 1 - j1:H - j0, i0:i1 + 1] = np.random.default_rng(b).standard_normal((j1 - j0 + 1, i1 - i0 + 1, C))
        dense = backward_f64.backward_with_bounds(v[b], f[b], px[b], gp, gb[b])
        wind = backward_f64.backward_with_bounds(v[b], f[b], px[b], gp, gb[b], window=win)
        assert wind[2] is None
        assert np.array_equal(dense[0], wind[0]) and np.array_equal(dense[1], wind[1])
        assert np.abs(dense[0]).sum() > 0 and np.abs(dense[1]).sum() > 0
        for k in ("S_v", "n_v", "S_c", "n_c", "N_v", "L_v", "clip_v", "clip_c", "n_half"):
            assert np.array_equal(getattr(dense[3], k), getattr(wind[3], k)), k
        assert np.array_equal(dense[2], np.where((gb[b] < 0)[..., None], gp, 0.0))
        if i0 == 0 and i1 == W - 1:
            continue
        with pytest.raises(AssertionError):  # the contract: zero outside the window
            backward_f64.backward(v[b], f[b], px[b], gp, gb[b], window=(i0, i1 - 1, j0, j1))


@pytest.mark.parametrize("name,window", lf.PAIRS, ids=["%s-%s" % p for p in lf.PAIRS])
def test_oracle_forward_windows(name, window):
    b = lf.bulk(name)
    lf.check_forward(name, window, b.px[0], b.gb[0], b.depth[0], b.bary[0], b.face[0])


@pytest.mark.parametrize("name,window", lf.PAIRS, ids=["%s-%s" % p for p in lf.PAIRS])
def test_oracle_backward_windows(name, window):
    b = lf.bulk(name)
    ref = lf.reference(name, window)
    gp = lf.cotangent(name, window)
    gv, gc, gbg = oracle.rasterise_bwd(*b.inputs[1:], b.px, gp, b.gb)
    assert np.all(gv[..., 2] == 0.0)
    print("\n" + bc.fmt("%s %s" % (name, window), bc.check_bound(gv, gc, ref, in_double=True)))
    assert np.array_equal(gbg, lf.background_cotangent(name, window, gp, b.gb))


@pytest.mark.parametrize("name,window", lf.SINGLE_PAIRS, ids=[p[1] for p in lf.SINGLE_PAIRS])
def test_oracle_large_edge_single_term(name, window):
    """A single pair term whose midpoint lies within 1/256 px of an edge of 2021 px (E_k >= 2^24 at the owner's
    pixel, |E2_k| <= E_k / 64; asserted by the case): the oracle converts the exact int64 E2_k and stays inside the
    bound that counts its roundings relative to the term."""
    b = lf.bulk(name)
    ref = lf.reference(name, window)
    gp = lf.cotangent(name, window)
    gv, gc, gbg = oracle.rasterise_bwd(*b.inputs[1:], b.px, gp, b.gb)
    print("\n" + bc.fmt(window, bc.check_bound(gv, gc, ref, in_double=True)))
    assert np.array_equal(gbg, lf.background_cotangent(name, window, gp, b.gb))
