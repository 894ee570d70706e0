"""CPU: the layout accessor (dirt_debug_layout) against dirt_workspace_sizes and DESIGN.md 2's formulas, and the
checker of tests/setup_state.py against itself: the statement encoded into `saved` / `scratch`-shaped bytes passes,
and each single mutation of those bytes that the GPU tests are meant to catch produces a finding."""
import numpy as np
import pytest

import scenes
import setup_state as ss

FRAMES = [(64, 64), (65, 63), (200, 136), (24, 8192), (2112, 8192)]  # (H, W) of tests/test_gpu_setup_state.py


def _align(v, a=256):
    return (v + a - 1) // a * a


@pytest.mark.parametrize("H,W", FRAMES + [(2048, 8192)])
@pytest.mark.parametrize("B,F,cap", [(1, 33, 0), (3, 129, 0), (2, 40, 1000), (1, 0, 0)])
def test_layout_accessor(H, W, B, F, cap):
    from dirt_amd import _lib
    L = _lib.debug_layout(B, H, W, F, cap)
    assert set(L) == set(_lib.LAYOUT_FIELDS)
    assert (L["saved_total"], L["scratch_total"]) == _lib.workspace_sizes(B, H, W, 1, 3 * F, F, cap)
    # coarse tiles of 64 px, doubled until the frame has at most 4096 of them
    cshift = 6
    while ((W + (1 << cshift) - 1) >> cshift) * ((H + (1 << cshift) - 1) >> cshift) > 4096:
        cshift += 1
    nctx, ncty = (W + (1 << cshift) - 1) >> cshift, (H + (1 << cshift) - 1) >> cshift
    assert (L["cshift"], L["nctx"], L["ncty"]) == (cshift, nctx, ncty)
    assert cshift == (7 if (H, W) == (2112, 8192) else 6)
    slabs = max(B * nctx * ncty, 1)
    assert L["nrec"] == 6 * F
    assert L["slab"] == (max(cap // slabs, 1) if cap > 0 else F + F // 4 + 64)  # (far below the 2^29-entry budget)
    assert L["saved_fdata"] == _align(B * 6 * F * 128)
    assert L["saved_cov"] == L["saved_fdata"] + _align(B * F * 32)
    assert L["saved_total"] == L["saved_cov"] + _align(B * H * W)
    assert L["off_count"] == 0
    assert L["off_flag"] == _align(2 * B * nctx * ncty * 4 * L["kCountStride"])
    assert L["off_bins"] == L["off_flag"] + 256
    assert L["scratch_total"] == L["off_bins"] + _align(L["slab"] * slabs * 8)
    consts = dict(kCountStride=64, kParP=16, kParQ=32, kStatCapCulled=48, kStatClamped=52, sizeof_Rec=128,
                  sizeof_FaceData=32, kRecBboxOffset=40, kFusedMaxF=32, kFusedMaxTiles=8192, kSmallPairs=8, kBigCap=64,
                  kBinThreads=256, kSetupSmallGrid=128)
    assert {k: L[k] for k in consts} == consts
    # the flag words lie inside the 256-B flag area, on lines of their own
    words = [0, L["kParP"], L["kParQ"], L["kStatCapCulled"], L["kStatClamped"]]
    assert all(0 <= w < ss.FLAG_WORDS for w in words) and len(set(words)) == 5
    assert ss.REC.itemsize == L["sizeof_Rec"] and ss.FACEDATA.itemsize == L["sizeof_FaceData"]
    assert ss.REC.fields["i0"][1] == L["kRecBboxOffset"]


def test_layout_accessor_rejects_a_bad_count():
    import ctypes
    from dirt_amd import _lib
    _lib.debug_layout(1, 64, 64, 33)  # (sets the signature)
    out = (ctypes.c_int64 * 64)()
    fn = _lib.load().dirt_debug_layout
    assert fn(1, 64, 64, 33, 0, out, len(_lib.LAYOUT_FIELDS) + 1) == _lib.DIRT_EINVAL
    assert fn(1, 64, 64, 33, 0, out, 3) == _lib.DIRT_OK and list(out[:4]) == [6, 1, 1, 0]


# ---- the checker against itself


def _scene():
    """clipping_scene at 200 x 136 (4 x 3 coarse tiles) plus the faces the mutations need: one out of range, one of
    zero area, one sloped and one flat ordinary face."""
    bg, v, c, f = scenes.clipping_scene(W=200, H=136)
    extra = np.array([[-0.5, -0.5, 0.1, 1.0], [0.6, -0.4, 0.3, 1.0], [0.1, 0.7, -0.2, 1.0],
                      [-0.2, -0.2, 0.25, 1.0], [0.3, -0.2, 0.25, 1.0], [0.0, 0.4, 0.25, 1.0]], np.float32)
    n = len(v)
    v = np.concatenate([v, extra])
    f = np.concatenate([f, [[n, n + 1, n + 2], [n + 3, n + 4, n + 5], [n, n, n + 1], [0, 1, len(v)]]]).astype(np.int32)
    return v, f, 200, 136


@pytest.fixture(scope="module")
def stated():
    from dirt_amd import _lib
    v, f, W, H = _scene()
    st = ss.frame_statement(v, f, W, H)
    B, F = 2, len(f)
    return _lib, st, B, F, H, W


def _encoded(stated, cap=0, binned=1):
    _lib, st, B, F, H, W = stated
    L = _lib.debug_layout(B, H, W, F, cap)
    ex = ss.Expect([st, st], binned=binned)
    saved, scratch = ss.encode(L, B, F, ex, np.random.default_rng(5))
    return L, ex, ss.decode(L, B, F, saved, scratch)


def test_scene_reaches_what_the_mutations_need(stated):
    _, st, _, F, _, _ = stated
    assert st.oob and F > 32
    kinds = {(r.empty, r.clipped) for r in st.records.values()}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    assert {nsub for _, _, nsub, _ in st.faces} >= {0, 1, 2, 3}
    assert any(r.plane() == "flat" for r in st.records.values() if not r.empty)
    assert max(len(t) for t in st.tiles(6).values()) >= 3 and len(st.tiles(6)) == 12


@pytest.mark.parametrize("binned", [1, 2, 3])
def test_encoded_statement_passes(stated, binned):
    L, ex, dec = _encoded(stated, binned=binned)
    found = ss.check(dec, ex)
    assert not found, found
    assert 0.0 < found.worst_plane <= 1.0 / 6.0  # (one rounding to float32 against a bound of six)


def test_encoded_statement_passes_with_overflowed_slabs(stated):
    L, ex, dec = _encoded(stated, cap=2 * 12 * 35)
    assert L["slab"] == 35
    n = [len(t) for t in ex.stmts[0].tiles(L["cshift"]).values()]
    assert max(n) > 35 >= min(n)  # some slabs overflow, some do not
    assert not ss.check(dec, ex)


def test_fused_state_passes_and_counts_are_held_to_zero(stated):
    L, ex, dec = _encoded(stated, binned=0)
    assert not ss.check(dec, ex)
    dec.counts[0, 1, 2] = 1
    assert ss.check(dec, ex)


def _tile(dec, ex, least=2):
    """A (frame 1, tile) with at least `least` entries, not overflowed."""
    tiles = ex.stmts[1].tiles(dec.L["cshift"])
    c = max(tiles, key=lambda c: len(tiles[c]))
    assert least <= len(tiles[c]) <= dec.L["slab"]
    return 1, c, len(tiles[c])


def _record(dec, ex, pred):
    return next(ri for ri, r in sorted(ex.stmts[1].records.items()) if pred(r))


def _mut_duplicate(dec, ex):
    b, c, n = _tile(dec, ex)
    dec.bins[b, c, 1] = dec.bins[b, c, 0]


def _mut_duplicate_and_count(dec, ex):
    b, c, n = _tile(dec, ex)
    dec.bins[b, c, n] = dec.bins[b, c, 0]
    dec.counts[0, b, c] += 1


def _mut_drop(dec, ex):
    b, c, n = _tile(dec, ex)
    dec.bins[b, c, 0] = dec.bins[b, c, n - 1]
    dec.counts[0, b, c] -= 1


def _mut_move_to_neighbour(dec, ex):
    tiles = ex.stmts[1].tiles(dec.L["cshift"])
    # an entry of tile c whose record does not touch tile c + 1, moved there
    c, ri = next((c, ri) for c in sorted(tiles) for ri in sorted(tiles[c]) if c + 1 in tiles and ri not in tiles[c + 1])
    n, m = len(tiles[c]), len(tiles[c + 1])
    pos = [int(x) for x in dec.bins[1, c]["ri"][:n]].index(ri)
    dec.bins[1, c + 1, m] = dec.bins[1, c, pos]
    dec.bins[1, c, pos] = dec.bins[1, c, n - 1]
    dec.counts[0, 1, c] -= 1
    dec.counts[0, 1, c + 1] += 1


def _mut_rel(delta_bit):
    def mut(dec, ex):
        # a record whose box ends inside the tile: i1 of rel_bbox one wider / narrower
        b, c, n = _tile(dec, ex)
        lim = (1 << dec.L["cshift"]) - 1
        k = next(k for k in range(n) if 0 < (int(dec.bins[b, c, k]["rel"]) >> 8 & 0xff) < lim)
        dec.bins[b, c, k]["rel"] = int(dec.bins[b, c, k]["rel"]) + (delta_bit << 8)
    return mut


def _mut_count(d):
    def mut(dec, ex):
        b, c, n = _tile(dec, ex)
        dec.counts[0, b, c] = int(dec.counts[0, b, c]) + d
    return mut


def _mut_idle(dec, ex):
    dec.counts[1, 0, 5] = 1


def _mut_swap_parity(dec, ex):
    L = dec.L
    dec.flag[L["kParP"]], dec.flag[L["kParQ"]] = dec.flag[L["kParQ"]], dec.flag[L["kParP"]]


def _mut_i1(dec, ex):
    dec.recs[1, _record(dec, ex, lambda r: not r.empty)]["i1"] += 1


def _mut_D(dec, ex):
    dec.recs[1, _record(dec, ex, lambda r: not r.empty)]["D"] *= -1


def _mut_za(dec, ex):
    ri = _record(dec, ex, lambda r: not r.empty and r.plane() not in (None, "flat"))
    exact, bound = ex.stmts[1].records[ri].plane()[0]
    dec.recs[1, ri]["za"] = np.float32(float(exact + 2 * bound))


def _mut_flat(dec, ex):
    dec.recs[1, _record(dec, ex, lambda r: not r.empty and r.plane() == "flat")]["zb"] = 2.0 ** -149


def _mut_z0(dec, ex):
    rec = dec.recs[1, _record(dec, ex, lambda r: not r.empty)]
    rec["z0"] = np.nextafter(rec["z0"], np.float32(2.0))


def _mut_basis(dec, ex):
    rec = dec.recs[1, _record(dec, ex, lambda r: not r.empty and r.clipped and r.s > 0)]
    rec["basis"][4] = np.nextafter(rec["basis"][4], np.float32(2.0))


def _mut_iw(dec, ex):
    rec = dec.recs[1, _record(dec, ex, lambda r: not r.empty and r.clipped)]
    rec["iw"][2] = np.nextafter(rec["iw"][2], np.float32(0.0))


def _face(ex, pred):
    return next(f for f, face in enumerate(ex.stmts[1].faces) if pred(*face))


def _mut_nsub(dec, ex):
    dec.fdata[1, _face(ex, lambda idx, q, nsub, clipped: nsub >= 2)]["nsub"] -= 1


def _mut_clipped(dec, ex):
    dec.fdata[1, _face(ex, lambda idx, q, nsub, clipped: clipped)]["clipped"] = 0


def _mut_q(dec, ex):
    # (w != 1: where 1 / w and w differ)
    fd = dec.fdata[1, _face(ex, lambda idx, q, nsub, clipped: nsub == 1 and not clipped and q[0] != 1.0)]
    fd["q"][0] = np.float32(1.0) / fd["q"][0]


def _mut_v(dec, ex):
    dec.fdata[1, 3]["v"][1] += 1


def _mut_empty_valid(dec, ex):
    rec = dec.recs[1, _record(dec, ex, lambda r: r.empty)]
    rec["i0"], rec["i1"], rec["j0"], rec["j1"] = 3, 4, 3, 4


def _mut_empty_face(dec, ex):
    dec.recs[1, _record(dec, ex, lambda r: r.empty)]["face"] += 1


def _mut_oob_flag(dec, ex):
    dec.flag[0] = 0


def _mut_clamp_counter(dec, ex):
    dec.flag[dec.L["kStatClamped"]] += 1


MUTATIONS = {
    "duplicated_entry": _mut_duplicate,
    "duplicated_entry_counted": _mut_duplicate_and_count,
    "dropped_entry": _mut_drop,
    "entry_moved_to_neighbour_tile": _mut_move_to_neighbour,
    "rel_bbox_wider": _mut_rel(1),
    "rel_bbox_narrower": _mut_rel(-1),
    "count_larger": _mut_count(1),
    "count_smaller": _mut_count(-1),
    "idle_count_set_nonzero": _mut_idle,
    "swapped_parity": _mut_swap_parity,
    "i1_off_by_one": _mut_i1,
    "D_negated": _mut_D,
    "za_twice_its_bound": _mut_za,
    "flat_record_sloped": _mut_flat,
    "z0_one_ulp": _mut_z0,
    "basis_one_ulp": _mut_basis,
    "iw_one_ulp": _mut_iw,
    "nsub_off_by_one": _mut_nsub,
    "clipped_flipped": _mut_clipped,
    "q_holds_w": _mut_q,
    "vertex_index_changed": _mut_v,
    "empty_record_with_valid_bbox": _mut_empty_valid,
    "empty_record_wrong_face": _mut_empty_face,
    "out_of_range_flag_cleared": _mut_oob_flag,
    "clamp_counter_off": _mut_clamp_counter,
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_reported(stated, name):
    L, ex, dec = _encoded(stated)
    before = (dec.recs.tobytes(), dec.fdata.tobytes(), dec.counts.tobytes(), dec.flag.tobytes(), dec.bins.tobytes())
    MUTATIONS[name](dec, ex)
    after = (dec.recs.tobytes(), dec.fdata.tobytes(), dec.counts.tobytes(), dec.flag.tobytes(), dec.bins.tobytes())
    assert before != after, "the mutation changed nothing"
    found = ss.check(dec, ex)
    print(name, "->", found[:3])
    assert found, "the checker missed: " + name


def test_overflowed_slab_mutations_are_reported(stated):
    """In a tile with more entries than its slab: a duplicate and a foreign entry are findings, a different subset
    of the tile's records is not."""
    L, ex, dec = _encoded(stated, cap=2 * 12 * 35)
    tiles = ex.stmts[0].tiles(L["cshift"])
    c = max(tiles, key=lambda c: len(tiles[c]))
    assert len(tiles[c]) > L["slab"]
    held = [int(x) for x in dec.bins[0, c]["ri"]]
    other = next(ri for ri in sorted(tiles[c]) if ri not in held)
    dec.bins[0, c, 0] = (other, tiles[c][other])
    assert not ss.check(dec, ex)
    dec.bins[0, c, 1] = dec.bins[0, c, 0]
    assert ss.check(dec, ex)
    L, ex, dec = _encoded(stated, cap=2 * 12 * 35)
    foreign = next(ri for ri, r in sorted(ex.stmts[0].records.items()) if not r.empty and ri not in tiles[c])
    dec.bins[0, c, 0]["ri"] = foreign
    assert ss.check(dec, ex)
    L, ex, dec = _encoded(stated, cap=2 * 12 * 35)
    dec.counts[0, 0, c] -= 1  # (the full count, not the number placed)
    assert ss.check(dec, ex)
