"""Exact statement of the forward of one frame.  TEST INFRASTRUCTURE ONLY.

A second, independent statement of depth, clipping, the visible record and the forward's values next to
oracle/dirt_oracle.c and the HIP kernels, which were written together and are compared bit for bit: an error
they share passes every parity test.  It shares geometry with tests/backward_f64.py (R1/R2 snapping and R5
clipping in numpy float32, R3 on Python integers) and no code or algebra with the oracle or dirt_amd/csrc.

Depth.  The exact depth of a covering record at a pixel centre is the plane through its snapped vertices,
    z* = sum_k E_k zw_k / D,
with the integer edge values E_k and zw_k R1's float32 window depths (dyadic rationals): one Python-integer
numerator over D 2^P, rounded once to float64.  It uses none of R4's za / zb / fma formulation.

What float32 R4 may return around z*.  R4 evaluates zw = fma(za, fx - fx0, fma(zb, fy - fy0, z0)) with
za = (dz1 dy2 - dz2 dy1) / det, zb = (dx1 dz2 - dx2 dz1) / det, dz_k = zw_k - zw_0, dx_k, dy_k the snapped
offsets in pixels, det = D / 65536.  Counting roundings (u = 2^-24, each relative to its own result):
    dz_k 1, dy_k (or dx_k) 1 (exact below 2^24 sub-pixel units, counted anyway), their product 1: 3 per term;
    the difference of the two products 1, relative to at most |term 1| + |term 2|;
    float(D) 1, the division 1                                   -> za, zb: 6 u (|term 1| + |term 2|) / |det|;
    fx - fx0, fy - fy0 exact (multiples of 2^-8 below 2^16);
    the inner fma 1, relative to at most Tb + |z0|; the outer fma 1, relative to at most Ta + Tb + |z0|,
with Ta = (|dz1 dy2| + |dz2 dy1|) / |det| |fx - fx0| and Tb = (|dx1 dz2| + |dx2 dz1|) / |det| |fy - fy0|.
Ta carries 6 + 1, Tb 6 + 2, |z0| 2, so with S = |z0| + Ta + Tb
    |zw - z*| <= e = K_DEPTH u S,   K_DEPTH = 8
(times 1 + 2^-20 for the second-order terms and the float64 evaluation of S and z*, plus 2^-100 for products
that underflow).  A record whose three zw are equal has dz = 0, za = zb = 0 and zw = z0 with no rounding at
all: e = 0.  A flat bound or sum |b_k zw_k| would be wrong: on slivers za and zb cancel.

Quantisation.  d = trunc(fl(zw (2^24 - 1) + 0.5)), one float32 rounding of the exact fma argument x.  Below
2^24 the float32 grid is no coarser than the integers, so d is floor(x) or floor(x) + 1: a record's 24-bit
depth lies in [floor(x(z* - e)), floor(x(z* + e)) + 1]; with e = 0 it is the exactly rounded value (`quantise`).
For zw >= 0.5 that rounding is to the nearest integer, ties to even: zw = 1 - 2^-24 gives x = 2^24 - 1.5 + 2^-24,
which rounds to 2^24 - 1 and fails `d < 2^24 - 1` like zw = 1 itself; 1 - 2^-23 is the largest visible zw.

Visibility.  A record is certainly / possibly in range when its whole interval / some of it satisfies
0 <= zw <= 1 and d < 2^24 - 1.  Record a is certainly beaten when a record b that is certainly in range has
d_hi(b) < d_lo(a), or d_hi(b) <= d_lo(a) and a lower (face, sub-triangle) key (R4: LESS, the lowest face wins
ties), or the same ordered (X, Y, zw) triples -- bit-identical R4 inputs, hence bit-identical depths -- and a
lower key.  The possible winners of a pixel are the possibly-in-range records not certainly beaten; the pixel
is decided when there is at most one.

Values of a visible record at a pixel centre, float64: the parent barycentrics lambda_i = sum_k mu_k basis_ki,
mu_k = (E_k / w_k) / sum_j (E_j / w_j) (`Tri.weights`), and the colour sum_i lambda_i c_i.  R6's roundings:
    a_k = float(E_k) * (1 / w_k): 3;  s = (a0 + a1) + a2, all a_k >= 0 inside a record, no cancellation: 3 + 2;
    1 / s: 6;  m_k = a_k * (1 / s): 3 + 6 + 1 = 10;  m_k basis_ki: 11;  the two additions: 2
    -> |lambda_i - exact| <= K_BARY u T_i,  T_i = sum_k |mu_k basis_ki|,  K_BARY = 13
       (a face that was not clipped has the identity basis: 10 would do; one constant is kept);
    lambda_i c_i: 14; the two additions: 2
    -> |colour - exact| <= K_COLOUR u sum_i T_i |c_i|,  K_COLOUR = 16.
The depth output is d / (2^24 - 1), one correctly rounded float32 division.

Measured |error| / (u sum |terms|) on the scene table (tests/forward_cases.py), oracle and HIP kernels alike:
depth 1.73 (a lower bound, read from d), barycentrics 4.79, colours 4.80 -- below the derived 8, 13 and 16.
"""
from fractions import Fraction

import numpy as np

import backward_f64
from backward_f64 import EXTRA_PER_FACE, GBUF_MULTI

U = 2.0 ** -24
DEPTH_MAX = (1 << 24) - 1
K_DEPTH, K_BARY, K_COLOUR = 8, 13, 16
SLACK = 1.0 + 2.0 ** -20


def record_index(F, f, s):
    """Sub-triangle 0 of face f is record f, sub-triangle s > 0 is record F + 5 f + s - 1."""
    return f if s == 0 else F + EXTRA_PER_FACE * f + s - 1


def quantise(zw):
    """R4's d = trunc(fl32(zw (2^24 - 1) + 0.5)) for an exact rational 0 <= zw <= 1, in exact arithmetic."""
    x = Fraction(zw) * DEPTH_MAX + Fraction(1, 2)
    e = 0
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    while Fraction(2) ** e > x:
        e -= 1
    q = x / Fraction(2) ** (e - 23)           # 2^23 <= q < 2^24: round to the nearest integer, ties to even
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return int(n * Fraction(2) ** (e - 23))   # trunc of the rounded float


class Frame:
    """The statement of one frame: per covering (pixel, record) pair, flat arrays sorted by nothing in
    particular -- pix (window j * W + i), rec, face, key (face * 8 + s), z (float64 of z*), S, d_lo, d_hi,
    certain, possible, winner -- and per pixel `winners[j][i]`, the list of pair indices that may be visible.

    window = (i0, i1, j0, j1), window coordinates, inclusive: the statement of those pixels only.  Record bounding
    boxes are intersected with it, `pix` is (j - j0) * (i1 - i0 + 1) + (i - i0) and the per-pixel tables (winners,
    any_certain, covered) are window-sized and indexed [j - j0][i - i0]; nothing of the frame's size is allocated,
    so the frame may be 8192x8192.  None is the whole frame."""

    def __init__(self, vertices, faces, W, H, record=None, window=None):
        self.W, self.H = W, H
        self.window = i0, i1, j0, j1 = (0, W - 1, 0, H - 1) if window is None else tuple(int(x) for x in window)
        assert 0 <= i0 <= i1 < W and 0 <= j0 <= j1 < H, self.window
        self.ww, self.wh = i1 - i0 + 1, j1 - j0 + 1
        self.vertices, self.faces = vertices, faces
        V, F = vertices.shape[0], faces.shape[0]
        self.F = F
        record = record or record_index
        self.tris = [backward_f64.setup_face(vertices, faces[f], V, W, H) for f in range(F)]
        cols = {k: [] for k in ("pix", "rec", "face", "key", "z", "S", "d_lo", "d_hi", "certain", "possible", "flat",
                                "triple")}
        self.rec_tri = {}
        triple_ids = {}
        for f, (subs, clipped) in enumerate(self.tris):
            for s, t in enumerate(subs):
                if t is None:
                    continue
                ri = record(F, f, s)
                self.rec_tri[ri] = (f, s, t, clipped)
                self._add_record(cols, ri, f, s, t, triple_ids)
        self.n = sum(len(a) for a in cols["pix"])
        for k, parts in cols.items():
            dt = {"z": float, "S": float, "certain": bool, "possible": bool, "flat": bool}.get(k, np.int64)
            setattr(self, k, np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt))
        self._resolve()

    def _add_record(self, cols, ri, f, s, t, triple_ids):
        wi0, wi1, wj0, wj1 = self.window
        i0, i1 = max(wi0, (min(t.X) - 128 + 255) // 256), min(wi1, (max(t.X) - 128) // 256)
        j0, j1 = max(wj0, (min(t.Y) - 128 + 255) // 256), min(wj1, (max(t.Y) - 128) // 256)
        if i0 > i1 or j0 > j1:
            return
        inside, E = t.covers_grid(i0, i1, j0, j1)
        if not inside.any():
            return
        jj, ii = np.nonzero(inside)
        n = len(ii)
        ii, jj = ii + i0, jj + j0
        cols["pix"].append((jj - wj0) * self.ww + (ii - wi0))
        cols["rec"].append(np.full(n, ri))
        cols["face"].append(np.full(n, f))
        cols["key"].append(np.full(n, f * 8 + s))
        triple = tuple((t.X[k], t.Y[k], float(t.zw[k])) for k in range(3))
        cols["triple"].append(np.full(n, triple_ids.setdefault(triple, len(triple_ids))))
        zw = [float(z) for z in t.zw]
        if not all(np.isfinite(z) for z in zw):
            # a non-finite zw makes R4's plane value infinite or NaN: never inside [0, 1]
            for k, v in (("z", np.nan), ("S", np.nan), ("d_lo", 0), ("d_hi", 0), ("certain", False), ("possible", False),
                         ("flat", False)):
                cols[k].append(np.full(n, v))
            return
        if zw[0] == zw[1] == zw[2]:
            ok = 0.0 <= zw[0] <= 1.0
            d = quantise(Fraction(zw[0])) if ok else 0
            ok = ok and d < DEPTH_MAX
            for k, v in (("z", zw[0]), ("S", abs(zw[0])), ("d_lo", d), ("d_hi", d), ("certain", ok), ("possible", ok),
                         ("flat", True)):
                cols[k].append(np.full(n, v))
            return
        # exact plane: zw_k = Z_k / 2^P, z* = sum E_k Z_k / (D 2^P), one rounding to float64
        fr = [Fraction(z) for z in zw]
        den = max(q.denominator for q in fr)
        Z = [int(q * den) for q in fr]
        Eo = [e[inside].astype(object) for e in E]
        num = Eo[0] * Z[0] + Eo[1] * Z[1] + Eo[2] * Z[2]
        z = np.array([int(a) / (t.D * den) for a in num], float)
        # S of R4's plane form (vertex 0 is the plane's origin; the orientation sign cancels in |.|)
        dz1, dz2 = zw[1] - zw[0], zw[2] - zw[0]
        dx1, dy1 = (t.X[1] - t.X[0]) / 256.0, (t.Y[1] - t.Y[0]) / 256.0
        dx2, dy2 = (t.X[2] - t.X[0]) / 256.0, (t.Y[2] - t.Y[0]) / 256.0
        det = t.D / 65536.0
        fx = np.abs((256 * ii + 128 - t.X[0]) / 256.0)
        fy = np.abs((256 * jj + 128 - t.Y[0]) / 256.0)
        S = abs(zw[0]) + (abs(dz1 * dy2) + abs(dz2 * dy1)) / det * fx + (abs(dx1 * dz2) + abs(dx2 * dz1)) / det * fy
        e = K_DEPTH * U * S * SLACK + 2.0 ** -100
        lo, hi = z - e, z + e
        tiny = 2.0 ** -20  # float64 evaluation of x = zw (2^24 - 1) + 0.5 near an integer
        d_lo = np.floor(np.clip(lo, 0.0, 1.0) * DEPTH_MAX + 0.5 - tiny).astype(np.int64)
        d_hi = np.floor(np.clip(hi, 0.0, 1.0) * DEPTH_MAX + 0.5 + tiny).astype(np.int64) + 1
        cols["z"].append(z)
        cols["S"].append(S)
        cols["d_lo"].append(np.maximum(d_lo, 0))
        cols["d_hi"].append(d_hi)
        cols["certain"].append((lo >= 0.0) & (hi <= 1.0) & (d_hi < DEPTH_MAX))
        cols["possible"].append((hi >= 0.0) & (lo <= 1.0) & (d_lo < DEPTH_MAX))
        cols["flat"].append(np.zeros(n, bool))

    def _resolve(self):
        W, H, n = self.ww, self.wh, self.n  # (the window's size: the per-pixel tables cover the window only)
        big = np.int64(1) << 62
        # per pixel: the smallest d_hi over the records certainly in range, and the lowest key among those
        m = np.full(W * H, big)
        cert = np.nonzero(self.certain)[0]
        np.minimum.at(m, self.pix[cert], self.d_hi[cert])
        kf = np.full(W * H, big)
        at_min = cert[self.d_hi[cert] == m[self.pix[cert]]]
        np.minimum.at(kf, self.pix[at_min], self.key[at_min])
        mp, kp = m[self.pix], kf[self.pix]
        beaten = (mp < self.d_lo) | ((mp <= self.d_lo) & (kp < self.key))
        # bit-identical R4 inputs: the lowest key among the certain records of a (pixel, triple) group wins
        group = {}
        for a in cert:
            g = (int(self.pix[a]), int(self.triple[a]))
            group[g] = min(group.get(g, big), int(self.key[a]))
        for a in range(n):
            g = group.get((int(self.pix[a]), int(self.triple[a])))
            if g is not None and g < self.key[a]:
                beaten[a] = True
        self.winner = self.possible & ~beaten
        self.any_certain = (m < big).reshape(H, W)
        self.covered = np.zeros(W * H, bool)
        self.covered[self.pix] = True
        self.covered = self.covered.reshape(H, W)
        self.winners = [[[] for _ in range(W)] for _ in range(H)]
        for a in np.nonzero(self.winner)[0]:
            p = int(self.pix[a])
            self.winners[p // W][p % W].append(int(a))

    def values(self, a, colours):
        """Of pair a: exact barycentrics, their bounds, colours [C], their bounds (float64)."""
        f, s, t, clipped = self.rec_tri[int(self.rec[a])]
        p = int(self.pix[a])
        i, j = self.window[0] + p % self.ww, self.window[2] + p // self.ww
        E = t.E(256 * i + 128, 256 * j + 128)
        lam, _ = t.weights([2 * e for e in E])
        q = [E[k] / t.w[k] for k in range(3)]
        sq = q[0] + q[1] + q[2]
        T = np.array([sum(abs(q[k] / sq * t.basis[k][i_]) for k in range(3)) for i_ in range(3)])
        c = colours[self.faces[f]].astype(np.float64)            # [3, C]
        lam = np.array(lam)
        return lam, K_BARY * U * T * SLACK, lam @ c, K_COLOUR * U * (T @ np.abs(c)) * SLACK


def check_frame(fr, background, colours, pixels, gbuffer=None, depth=None, barycentrics=None, face_ids=None):
    """Every assertion of the pin on one frame's outputs (rows top first; depth, barycentrics and one of gbuffer /
    face_ids may be None).  Returns the figures: worst |error| / (u sum |terms|) for depth (a lower bound of it,
    from d alone), barycentrics and colours -- to compare with K_DEPTH, K_BARY, K_COLOUR -- and the counts of
    covered and undecided pixels.  A windowed Frame: the outputs are the whole frame's, the window's pixels are
    visited and counted."""
    H = fr.H
    i0, i1, j0, j1 = fr.window
    worst = {"depth": 0.0, "barycentrics": 0.0, "colours": 0.0}
    undecided = 0
    for j in range(j0, j1 + 1):
        r = H - 1 - j
        for i in range(i0, i1 + 1):
            win = fr.winners[j - j0][i - i0]
            undecided += len(win) > 1
            where = "pixel (%d, %d)" % (i, j)
            seen_face = None
            if gbuffer is not None:
                word = int(gbuffer[r, i])
                if word >= 0:
                    ri = word & (GBUF_MULTI - 1)
                    assert ri in fr.rec_tri, "%s: record %d does not exist" % (where, ri)
                    seen_face = fr.rec_tri[ri][0]
                    assert bool(word & GBUF_MULTI) == fr.rec_tri[ri][3], "%s: clipped bit" % where
                else:
                    assert word == -1, where
                if face_ids is not None:
                    assert int(face_ids[r, i]) == (-1 if seen_face is None else seen_face), "%s: face id" % where
            elif face_ids[r, i] >= 0:
                seen_face = int(face_ids[r, i])
            if seen_face is None:
                assert not fr.any_certain[j - j0, i - i0], "%s: background, but a record is certainly in range" % where
                assert np.array_equal(pixels[r, i].view(np.uint32), background[r, i].view(np.uint32)), where
                if depth is not None:
                    assert depth[r, i] == np.float32(1.0), where
                if barycentrics is not None:
                    assert np.all(barycentrics[r, i] == 0.0), where
                continue
            if gbuffer is not None:
                mine = [a for a in win if fr.rec[a] == ri]
            else:
                mine = [a for a in win if fr.face[a] == seen_face]
            assert mine, "%s: face %d is not a possible winner %s" % (where, seen_face, [int(fr.rec[a]) for a in win])
            if len(win) == 1 and gbuffer is not None:
                expect = int(fr.rec[win[0]]) | (GBUF_MULTI if fr.rec_tri[int(fr.rec[win[0]])][3] else 0)
                assert word == expect, "%s: g-buffer word %#x, statement %#x" % (where, word, expect)
            if len(mine) > 1:
                continue  # two sub-triangles of one face and no g-buffer word to tell them apart
            a = mine[0]
            if depth is not None:
                y = depth[r, i]
                c = int(np.floor(float(y) * DEPTH_MAX))
                ds = [d for d in (c, c + 1) if np.float32(d) / np.float32(DEPTH_MAX) == y]
                assert ds, "%s: depth %r is no d / (2^24 - 1)" % (where, y)
                d = ds[0]
                assert fr.d_lo[a] <= d <= fr.d_hi[a] and d < DEPTH_MAX, "%s: d %d outside [%d, %d]" % (
                    where, d, fr.d_lo[a], fr.d_hi[a])
                if not fr.flat[a]:
                    x = fr.z[a] * DEPTH_MAX + 0.5
                    worst["depth"] = max(worst["depth"], max(abs(d - x) - 1.0, 0.0) / DEPTH_MAX / (U * fr.S[a]))
            lam, lam_b, col, col_b = fr.values(a, colours)
            if barycentrics is not None:
                err = np.abs(barycentrics[r, i].astype(np.float64) - lam)
                assert np.all(err <= lam_b), "%s: barycentrics off by %s, bound %s" % (where, err, lam_b)
                worst["barycentrics"] = max(worst["barycentrics"], float(np.max(err / np.maximum(lam_b, 1e-300)))
                                            * K_BARY)
            err = np.abs(pixels[r, i].astype(np.float64) - col)
            assert np.all(err <= col_b), "%s: colours off by %s, bound %s" % (where, err, col_b)
            nz = col_b > 0
            if nz.any():
                worst["colours"] = max(worst["colours"], float(np.max(err[nz] / col_b[nz])) * K_COLOUR)
    covered = int(fr.covered.sum())
    return dict(worst, covered=covered, undecided=undecided, share=undecided / max(covered, 1))
