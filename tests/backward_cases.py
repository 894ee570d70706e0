"""Case table and per-element contract of the backward's float64 pin.  TEST INFRASTRUCTURE ONLY.

Shared by tests/test_backward_f64.py (the oracle, on a CPU) and tests/test_gpu_backward_bound.py (the HIP kernel).

The contract.  tests/backward_f64.py states the gradient in float64 and, next to every element g of grad_vertices
and grad_vertex_colors, the sum S of the absolute values of its terms and their number n (backward_f64.Bounds).
With u = 2^-24, float32's unit roundoff:

    |got - g| <= (n - 1 + k) u S        (exactly 0 where S == 0)
    grad_vertices[..., 3] additionally + 4 u N (below);  sums kept in double: k u S + u |g| / 2 (the final cast).

n - 1 additions, each rounding a partial sum that is at most S in magnitude, cover every summation order: the DPP
run scans, the LDS tail ranges, the flush and the float atomics across tiles of grad_kernel.h, and a gather design
alike.  k counts the float32 roundings ONE term passes through before it is summed, each a relative error u of a
quantity whose magnitude is at most the absolute term; it is counted below from grad_kernel.h (K5) and
oracle/dirt_oracle.c (add_pair_owner, parent_lambda), the larger count taken, nothing fitted.

Pair term  omega s half (E2_k / 2D) (1 / w_k) [basis_ki] [x_ndc]  into dL/dx_i, dL/dy_i, dL/dw_i:
    s = -0.5 sum_c (G_c(p) + G_c(q)) (I_c(q) - I_c(p))   the add, the subtract and the product of a channel (3,
                                                         each relative to (|G(p)| + |G(q)|) |I(q) - I(p)|), C - 1
                                                         channel additions (the first adds to 0); -0.5 is exact  C + 2
    omega s half / 2D                                    K5: (float) D, 0.5 / D, s half (omega, code = 1, 2 exact),
                                                         times h2d (the fast path: half h2d 0.5, times code s)       4
                                                         oracle: s half, (float) 2D, the division                 (3)
    E_k(p)                                               int32 -> float (records with |A|, |B| < 2^14): exact
                                                         below 2^24; from there on |step| < 2^22 <= E_k(p) / 4, so
                                                         E2_k >= 1.75 E_k(p) and the conversion's u E_k(p) stays
                                                         within 1.15 u E2_k                                        2
                                                         int64 -> float by fast_i64_to_f32: (float) lo and the
                                                         fma, each relative to E_k(p) >= 0 (the pixel is covered,
                                                         so hi >= 0 and lo <= E_k(p)); see "Open" below          (2)
    the step 256 A_k (256 B_k)                           (float) A_k rounds from 2^24 on (clamped sub-vertices)      1
    E2_k = 2 E_k(p) + step                               one addition, relative to its result (the oracle converts
                                                         the exact int64 E2_k)                                       1
    1 / w_k                                              setup's IEEE division (bit-identical on every side:
                                                         -ffp-contract=off and the correctly rounded divide flag)    1
    E2_k (1 / w_k),  times the coefficient               two products                                                2
    x_ndc:  the subtraction mid (2 / W) - 1 (relative to |x_ndc|) and the product g x_ndc                            2
                                                                                              k_v = C + 15
    clipped records: the nine sub-vertex sums of a pixel mapped through the basis,
    (b_0i s_0 + b_1i s_1) + b_2i s_2: a product and two additions                                                 + 3
The sub-vertex w_k and basis_ki of a clipped record are inputs: the statement clips in float32 itself (R5), one IEEE
operation at a time like the oracle and the kernels (built with -ffp-contract=off; their records equal the oracle's,
tests/test_gpu_parity.py's bit-exact g-buffers and pixels), so no rounding separates them.
x_ndc(M) = mid (2 / W) - 1 has two roundings that are relative to mid (2 / W) <= 2, not to |x_ndc|: (float)(2 / W)
and the product (the oracle: one division mid / half).  They are an absolute error of at most 4 u in x_ndc, hence
4 u N in the w component, N = sum of the absolute dL/dx and dL/dy terms whose products with x_ndc, y_ndc the element
sums (Bounds.N_v).  Exact, and N's share zero, wherever 2 / W is a power of two.

Found by this contract and fixed in grad_kernel.h: the branch-free path folded the two pairs of an axis into
(c_0 + c_1) P_k + (c_0 - c_1) Q_k, P_k = 2 E_k(p) / w_k, Q_k = 256 A_k / w_k, rounding P_k and Q_k apart; where a pair's
midpoint lies within a pixel of the edge opposite vertex k (E2_k = 2 E_k(p) - 256 A_k ~ 0) the term lost
(|P_k| + |Q_k|) / |P_k - Q_k| times its own rounding: 74 and 132 on the single-term elements of channels_2 and
frame_17x33, 42 u S where k allows 18.  The path now forms each pair's E2_k first, as the general path does.
The int64 path, stated as the kernel computes it: records with |A_k| or |B_k| >= 2^14 convert E_k(o)
at the owner's pixel o before the pair's midpoint value E2_k = 2 E_k(o) +- step is formed, so fast_i64_to_f32's two
roundings are relative to E_k(o), not to E2_k: an error of at most 4 u E_k(o) in E2_k.  Where |E2_k| >= 2 E_k(o) (the
pair that leads away from the edge opposite k) that is within 2 u |E2_k|, the "2" the count above gives E_k(p), and the
count holds as it stands.  Where |E2_k| < 2 E_k(o) it does not, and not at all where E_k(o) >= 2^24 and the midpoint
lies within a pixel of the edge opposite k (edges of 256 px or more).  The kernel's bound therefore carries, for every
sub-vertex k of a term on that path with |E2_k| < 2 E_k(o), and for that term's elements only, the allowance
    2 u E_k(o) |d term / d E_k(o)| = 4 u E_k(o) omega S_pair half |basis_ki| / (2 D w_k)
(Bounds.L_v: E_k(o) is an integer the statement has, so the allowance is exact); the oracle converts the exact int64
E2_k and gets none.  Every other element -- without a term on that path, or with such terms only at |E2_k| >= 2 E_k(o)
-- keeps the bound above and is asserted against it.  Measured on large_frame_cases.SINGLE (single-term elements,
E_k(o) >= 2^24, |E2_k| <= E_k(o) / 64, L = 323 S): the kernel reaches 4.7 times the bound above and 0.13 of the bound
with the allowance; the oracle 0.08 of the bound above.

Colour term  lambda_i(p) G_c(p), lambda_i = sum_k mu_k basis_ki, mu_k = a_k / (a_0 + a_1 + a_2), a_k = E_k(p) / w_k
(every a_k >= 0 inside the record: nothing cancels):
    a_k: E_k(p) (2), 1 / w_k (1), the product (1)                                                                    4
    a_0 + a_1 + a_2: the same 4 in each operand, two additions                                                       6
    the reciprocal: v_rcp_f32, 1 ulp = 2 u (the CDNA ISA guide's accuracy statement for V_RCP_F32;
    the oracle divides: 1)                                                                                           2
    a_k rs,  times G_c(p)                                                                                            2
                                                                                              k_c = 14
    clipped records: (m_0 b_0i + m_1 b_1i) + m_2 b_2i                                                             + 3

Each case names the kernel path it is there for; where the path depends on the content, `condition` asserts it from
the oracle's g-buffer for the four tile geometries the kernel can be built with (TWX in {16, 32}, TH in {16, 8}).
Frames are at most 64x48 and batches at most 2 (the statement is pure-Python loops).
"""
import functools

import numpy as np

import backward_f64
import scenes
from oracle import oracle

U = backward_f64.U32
TILE_GEOMETRIES = [(16, 16), (32, 16), (16, 8), (32, 8)]
K_SLOTS = 64          # grad_kernel.h kSlots
SMALL_EDGE = backward_f64.INT64_EDGE  # grad_kernel.h kGradSmallEdge (the one copy: Bounds.L_v uses it too)
MULTI = backward_f64.GBUF_MULTI


def k_vertices(C, clipped):
    return C + 15 + 3 * np.asarray(clipped, np.int64)


def k_colours(clipped):
    return 14 + 3 * np.asarray(clipped, np.int64)


def tail_cap(twx, th, C):
    """grad_kernel.h kTailCap for the full gradient (GM = 3) at C = 1, 3, 7 (specialised kernels)."""
    cp = 4 if C == 3 else 8 if 4 < C <= 8 else C
    return 2 * (twx + 2) * (th + 2) * cp // (9 + 3 * C)


class Reference:
    """One case's inputs, the oracle's forward (the g-buffer is the statement's input) and the float64 statement
    with its bounds.  Computed once per case (reference()); nothing in it is modified afterwards."""

    def __init__(self, inputs, seed, keep_terms=False, forward=None, grad_pixels=None):
        self.inputs = bg, v, c, f = tuple(inputs)
        if bg.ndim == 3:
            self.inputs = bg, v, c, f = bg[None], v[None], c[None], f[None]
        self.gp = grad_pixels if grad_pixels is not None else \
            np.random.default_rng(seed).standard_normal(bg.shape).astype(np.float32)
        self.px, self.gb = forward if forward is not None else oracle.rasterise_fwd(bg, v, c, f)[:2]
        self.gv, self.gc, self.gbg, self.bounds = backward_f64.backward_batch_with_bounds(
            v, f, self.px, self.gp, self.gb, keep_terms)
        for name in ("S_v", "n_v", "S_c", "n_c", "N_v", "L_v", "clip_v", "clip_c"):
            setattr(self, name, backward_f64.stack_bounds(self.bounds, name))
        self.C = bg.shape[-1]
        for a in (self.gp, self.px, self.gb, self.gv, self.gc, self.gbg) + self.inputs:
            a.setflags(write=False)

    def bound_vertices(self, in_double=False):
        k = k_vertices(self.C, self.clip_v)
        if in_double:
            return k * U * self.S_v + 0.5 * U * np.abs(self.gv) + 4 * U * self.N_v
        return (np.maximum(self.n_v - 1, 0) + k) * U * self.S_v + 4 * U * self.N_v + 2 * U * self.L_v

    def bound_colours(self, in_double=False):
        k = k_colours(self.clip_c)
        if in_double:
            return k * U * self.S_c + 0.5 * U * np.abs(self.gc)
        return (np.maximum(self.n_c - 1, 0) + k) * U * self.S_c


def check_bound(got_v, got_c, ref, in_double=False, extra_v=0.0, extra_c=0.0, base_v=0.0, base_c=0.0):
    """The per-element contract for whichever of got_v / got_c is given; returns the worst error / bound ratios
    (and, for the record, the worst error / (u S)).  extra_*: added to the bound (the accumulate flag's own);
    base_*: what the sum started from."""
    out = {}
    for name, got, want, S, bound, extra, base in (
            ("grad_vertices", got_v, ref.gv, ref.S_v, ref.bound_vertices(in_double), extra_v, base_v),
            ("grad_vertex_colors", got_c, ref.gc, ref.S_c, ref.bound_colours(in_double), extra_c, base_c)):
        if got is None:
            continue
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape
        assert np.all(np.isfinite(got)), "%s: non-finite elements" % name
        err = np.abs(got - (want + base))
        zero = S == 0.0
        assert np.all(err[zero] == 0.0), "%s: %d elements without terms are not exact" % (name, (err[zero] != 0).sum())
        tot = bound + extra
        bad = err > tot
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, tot))
            units = np.where(zero, 0.0, err / np.where(zero, 1.0, U * S))
        out[name] = (float(ratio.max()) if ratio.size else 0.0, float(units.max()) if units.size else 0.0)
        if name == "grad_vertices" and ratio.size:  # for the record: against the bound without x_ndc's 4 u N
            plain = tot - 4 * U * ref.N_v
            out["(without 4 u N"] = (float(np.where(zero, 0.0, err / np.where(zero, 1.0, plain)).max()), 0.0)
        assert not bad.any(), "%s: %d of %d elements over the bound, worst %.3g of it at %s (error %.3g, S %.3g, n %d)" % (
            name, bad.sum(), (~zero).sum(), ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape),
            err.flat[np.argmax(ratio)], S.flat[np.argmax(ratio)],
            (ref.n_v if name == "grad_vertices" else ref.n_c).flat[np.argmax(ratio)])
    return out


def check_background(got_bg, ref):
    """grad_background: the cotangent exactly on uncovered pixels, 0 elsewhere."""
    want = np.where((ref.gb < 0)[..., None], ref.gp, np.float32(0.0))
    np.testing.assert_array_equal(got_bg, want)
    np.testing.assert_array_equal(ref.gbg.astype(np.float32), want)


def fmt(name, ratios):
    return "%-34s " % name + "  ".join(("%s %.3f)" % (k, v[0])) if k.startswith("(") else
                                       "%s %.3f of the bound (%.2f u S)" % ((k,) + v) for k, v in ratios.items())


# ---- conditions on the content (from the oracle's g-buffer, window order: row j of gw is window row j) --------------
def _window(gb):
    return gb[::-1]


def _records(gw):
    return np.where(gw < 0, -1, gw & (MULTI - 1))


def cond_cross_tile_pairs(ref):
    """Pairs whose two pixels lie in different tiles and show different records, across both kinds of border."""
    for b in range(ref.gb.shape[0]):
        r = _records(_window(ref.gb[b]))
        H, W = r.shape
        for twx, th in TILE_GEOMETRIES:
            xs = [x for x in range(twx - 1, W - 1, twx)]
            ys = [y for y in range(th - 1, H - 1, th)]
            if xs:
                assert any((r[:, x] != r[:, x + 1]).any() for x in xs), (twx, th)
            if ys:
                assert any((r[y] != r[y + 1]).any() for y in ys), (twx, th)


def cond_slot_overflow(ref):
    """More than kSlots distinct visible records in every aligned 16x8 block (so in every tile of every geometry)."""
    r = _records(_window(ref.gb[0]))
    H, W = r.shape
    for y in range(0, H - 7, 8):
        for x in range(0, W - 15, 16):
            blk = r[y:y + 8, x:x + 16]
            assert len(np.unique(blk[blk >= 0])) > K_SLOTS, (x, y)


def cond_tail_overflow(ref):
    """At most kSlots distinct records in every tile, and in some tile more run tails (runs of one record along a
    16-lane row) than kTailCap."""
    r = _records(_window(ref.gb[0]))
    H, W = r.shape
    for twx, th in TILE_GEOMETRIES:
        worst = 0
        for y in range(0, H, th):
            for x in range(0, W, twx):
                blk = r[y:y + th, x:x + twx]
                assert len(np.unique(blk[blk >= 0])) <= K_SLOTS
                runs = 0
                for row in blk:
                    for x16 in range(0, len(row), 16):
                        seg = row[x16:x16 + 16]
                        runs += int(((seg >= 0) & np.concatenate([[True], seg[1:] != seg[:-1]])).sum())
                worst = max(worst, runs)
        assert worst > tail_cap(twx, th, ref.C), (twx, th, worst, tail_cap(twx, th, ref.C))


def _visible_tris(ref, b=0):
    bg, v, c, f = ref.inputs
    H, W = ref.gb.shape[1:]
    F = f.shape[1]
    tris = {}
    for ri in np.unique(_records(ref.gb[b])):
        if ri >= 0:
            face = ri if ri < F else (ri - F) // backward_f64.EXTRA_PER_FACE
            sub = 0 if ri < F else (ri - F) % backward_f64.EXTRA_PER_FACE + 1
            tris[int(ri)] = backward_f64.setup_face(v[b], f[b][face], v.shape[1], W, H)[0][sub]
    return tris


def _cond_large(ref, want_hi):
    tris = _visible_tris(ref)
    large = {ri for ri, t in tris.items() if max(abs(x) for x in t.A + t.B) >= SMALL_EDGE}
    assert large and len(large) < len(tris)
    r = _records(_window(ref.gb[0]))
    H, W = r.shape
    for twx, th in TILE_GEOMETRIES:  # a tile showing large and small records
        assert any(len(set(np.unique(blk)) & large) and len(set(np.unique(blk[blk >= 0])) - large)
                   for y in range(0, H, th) for x in range(0, W, twx) for blk in [r[y:y + th, x:x + twx]])
    if want_hi:  # an edge value past 2^32 at a pixel the record covers: fast_i64_to_f32 with hi != 0
        js, is_ = np.nonzero(np.isin(r, list(large)))
        assert any(max(tris[int(r[j, i])].E(256 * i + 128, 256 * j + 128)) >= 2 ** 32 for j, i in zip(js, is_))


def cond_large_records(ref):
    _cond_large(ref, False)


def cond_far_records(ref):
    _cond_large(ref, True)


def cond_clipped_visible(ref):
    assert ((ref.gb >= 0) & ((ref.gb & MULTI) != 0)).any()


def cond_half_splits(ref):
    assert sum(b.n_half for b in ref.bounds) > 0


def cond_edge_on_pixel_centres(ref):
    tris = _visible_tris(ref)
    r = _records(_window(ref.gb[0]))
    js, is_ = np.nonzero(r >= 0)
    assert any(min(tris[int(r[j, i])].E(256 * i + 128, 256 * j + 128)) == 0 for j, i in zip(js, is_))
    cond_half_splits(ref)


def cond_high_valence(ref):
    bg, v, c, f = ref.inputs
    assert (f[0] == 0).any(axis=1).sum() >= 64
    assert ref.n_v[0, 0, 0] >= 300 and ref.n_v[0, 0, 3] >= 300, ref.n_v[0, 0]
    r = _records(_window(ref.gb[0]))
    H, W = r.shape
    for twx, th in TILE_GEOMETRIES:
        assert sum(bool((blk >= 0).any()) for y in range(0, H, th) for x in range(0, W, twx)
                   for blk in [r[y:y + th, x:x + twx]]) >= 3


def cond_non_finite_silhouette(ref):
    """Covered pixels next to background pixels holding a non-finite value (pairs that carry nothing), and pairs
    that do carry something elsewhere."""
    bad = (ref.gb[0] < 0) & ~np.isfinite(ref.px[0]).all(-1)
    cov = ref.gb[0] >= 0
    assert (bad[:, 1:] & cov[:, :-1]).any() and (bad[1:] & cov[:-1]).any()
    assert ref.n_v.sum() > 0


def cond_batch_differs(ref):
    assert ref.gb.shape[0] == 2 and not np.array_equal(ref.gb[0], ref.gb[1])


class Case:
    def __init__(self, name, path, build, condition=None, seed=1):
        self.name, self.path, self.build, self.condition, self.seed = name, path, build, condition, seed

    def __repr__(self):
        return self.name


def _bg(scene, value, C=None):
    bg, v, c, f = scene
    bg = bg.copy()
    bg[...] = value
    return bg, v, c, f


def _mixed_bg(scene):
    """-inf, +inf and NaN in thirds of the background, one channel of each pixel only."""
    bg, v, c, f = scene
    bg = bg.copy()
    W = bg.shape[1]
    bg[:, :W // 3, 0] = -np.inf
    bg[:, W // 3:2 * W // 3, -1] = np.inf
    bg[:, 2 * W // 3:, 0] = np.nan
    return bg, v, c, f


def _two_meshes():
    a = scenes.shared_mesh_scene(W=33, H=17, C=3, seed=5, n=4)
    b = scenes.fan_scene(W=33, H=17, C=3, seed=6, n=12, radius=7.0)
    V, F = max(a[1].shape[0], b[1].shape[0]), max(a[3].shape[0], b[3].shape[0])
    out = []
    for bg, v, c, f in (a, b):
        out.append((bg, np.concatenate([v, np.tile(v[:1], (V - len(v), 1))]),
                    np.concatenate([c, np.tile(c[:1], (V - len(c), 1))]),
                    np.concatenate([f, np.zeros((F - len(f), 3), np.int32)])))  # (padding faces 0, 0, 0: zero area)
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def _small(W, H, C=3, seed=0, perspective=False):
    return lambda: scenes.random_triangles(F=40, W=W, H=H, C=C, radius_px=max(2.0, min(6.0, min(W, H) / 2.0)),
                                           seed=seed, perspective=perspective)


CASES = [Case("frame_%dx%d" % (W, H), "tile borders and halos: frame smaller than / not a multiple of the tile",
              _small(W, H, seed=W * 100 + H), cond_cross_tile_pairs if min(W, H) > 16 else None)
         for W, H in ((16, 16), (15, 15), (17, 33), (33, 17), (1, 17), (17, 1))]
CASES += [
    Case("frame_64x48", "tile borders and halos: several tiles in both directions",
         lambda: scenes.random_triangles(F=120, W=64, H=48, radius_px=7.0, seed=2, perspective=True),
         cond_cross_tile_pairs),
    Case("tile_border_mesh", "silhouette and shared edges along x = 16, 32 and y = 8, 16",
         lambda: scenes.tile_border_mesh_scene(), cond_cross_tile_pairs),
]
CASES += [Case("channels_%d" % C, "channel class C = %d" % C, _small(33, 17, C=C, seed=77, perspective=True))
          for C in (1, 2, 3, 4, 5, 7, 8)]
CASES += [Case("slot_overflow_c%d" % C, "slot-table overflow (kNoSlot): a record per pixel",
               functools.partial(scenes.pixel_triangles_scene, C=C, seed=C), cond_slot_overflow) for C in (3, 7)]
CASES += [Case("tail_overflow_c%d" % C, "tail-cap overflow with few records: one-pixel stripes",
               functools.partial(scenes.stripe_scene, C=C, seed=C), cond_tail_overflow) for C in (3, 7)]
CASES += [
    Case("large_records", "edges of 64 px or more: the int64 edge path next to small records",
         lambda: scenes.large_record_scene(), cond_large_records),
    Case("far_records", "triangles reaching far outside the frame inside the guard band (edge values past 2^32)",
         lambda: scenes.large_record_scene(far=True, seed=3), cond_far_records),
    Case("clipping_scene", "clipped (multi) records", lambda: scenes.clipping_scene(W=64, H=48), cond_clipped_visible),
]
CASES += [Case("clipped_sliver_%d" % s, "clipped (multi) slivers", functools.partial(scenes.clipped_sliver_scene, s),
               cond_clipped_visible, seed=s) for s in (0, 7, 14)]
CASES += [
    Case("near_w0_41533", "clipped records around w = 0, the vertex cap",
         lambda: scenes.near_w0_scene(41533, W=33, H=17, C=1), cond_clipped_visible, seed=41533),
    Case("fuzz_167059", "dominant sliver; clipped sub-vertex beyond the guard band; batch of two",
         lambda: scenes.fuzz_case(167059), cond_clipped_visible, seed=167059),
    Case("fuzz_37851", "dominant sliver (1811-unit), C = 5, batch of two 64x48 frames",
         lambda: scenes.fuzz_case(37851), cond_clipped_visible, seed=37851),
    Case("abutting_edges", "ownership: abutting coplanar edges split 0.5 / 0.5",
         lambda: scenes.shared_mesh_scene(W=33, H=17, n=5), cond_half_splits),
    Case("interpenetrating", "ownership: interpenetrating pairs",
         lambda: scenes.interpenetrating_scene(3, W=33, H=17, pairs=3), cond_half_splits),
    Case("edge_on_pixel_centres", "ownership: face edges exactly on pixel centres (top-left rule)",
         lambda: scenes.pixel_centre_edge_scene(), cond_edge_on_pixel_centres),
    Case("high_valence_fan", "one vertex shared by 64 faces over several tiles: many atomics into one address",
         lambda: scenes.fan_scene(), cond_high_valence),
    Case("background_minus_inf", "non-finite background: -inf",
         lambda: _bg(scenes.shared_mesh_scene(W=33, H=17, n=5), -np.inf), cond_non_finite_silhouette),
    Case("background_plus_inf", "non-finite background: +inf",
         lambda: _bg(scenes.shared_mesh_scene(W=33, H=17, n=5), np.inf), cond_non_finite_silhouette),
    Case("background_nan_mixed", "non-finite background: NaN, -inf and +inf in single channels",
         lambda: _mixed_bg(scenes.fan_scene(W=33, H=17, n=9, radius=6.0)), cond_non_finite_silhouette),
    Case("batch_two_meshes", "B = 2 with different meshes per frame", _two_meshes, cond_batch_differs),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def reference(name, keep_terms=False):
    case = BY_NAME[name]
    ref = Reference(case.build(), case.seed, keep_terms)
    if case.condition is not None:
        case.condition(ref)
    return ref
