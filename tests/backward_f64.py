"""Float64 restatement of the registered gradient.  TEST INFRASTRUCTURE ONLY.

An independent statement of the backward next to oracle/dirt_oracle.c (C, float32 contributions summed in
double) and the HIP kernel (float32, atomics): it is written from the specification, in the specification's
own terms, and shares no code or algebra with either --
  * geometry: R1/R2 snapping and R5 clipping (Sutherland-Hodgman against z >= -w and the guard planes, in
    float32, carrying the parent barycentric basis, fan-triangulated) define the rasterised (sub-)triangles,
    whose edge functions are Python integers (R3);
  * pair scalar: s = -0.5 sum_c (G_c(p) + G_c(q)) (I_c(q) - I_c(p)) for horizontally / vertically adjacent
    pixels p < q (window order), in float64; pairs touching a background pixel with a non-finite value carry
    nothing;
  * ownership: the common face; the only face if the other side is background; else the exact coverage tests
    covers(f, q) / covers(g, p) decide whose edge separates the pixels (weight 1), 0.5 / 0.5 when ambiguous;
  * weights: the owner's perspective-correct barycentrics at the pair midpoint M -- screen-space barycentrics
    b_k = E_k(M) / D of the record's snapped vertices, mu_k = (b_k / w_k) / sum_j (b_j / w_j) with the
    record's own clip w, mapped to the parent's vertices through the clip basis (identity for faces that did
    not take the clipping path): lambda_i = sum_k mu_k basis_ki; Wm = sum_k mu_k w_k, the clip w of M on the
    rasterised triangle;
  * chain rule through xw = (x / w + 1) W / 2: dL/dx_i += omega s (W/2) lambda_i / Wm and
    dL/dw_i -= omega s (W/2) lambda_i x_ndc(M) / Wm (x pairs; y pairs with H and y); dL/dz = 0;
  * colours: dL/dc_v += lambda_v(p) G(p) at the pixel centre of every covered pixel; dL/dbackground = G on
    uncovered pixels.
The visible record of each pixel (the forward's g-buffer) is an input: visibility is the forward's output,
pinned separately -- coverage by tests/exact_cover.py, depth, clipping, the visible record and the forward's
values by tests/forward_exact.py (exact plane depth with derived float32 bounds; the oracle against it in
tests/test_forward_exact.py, the HIP kernels in tests/test_gpu_forward_exact.py).  Pure-Python loops: small
frames, or a small window of a large one (`window`).

backward_with_bounds / backward_batch_with_bounds return the same values and, per element, the sum of the absolute
values of its terms and their number (Bounds): what the per-element contract of tests/backward_cases.py is stated in.
"""
import numpy as np

F32 = np.float32
GBUF_MULTI = 1 << 30
EXTRA_PER_FACE = 5


def _guard_clamp(xn, g):
    """R5 sub-vertex clamp: x/w of a clipped face's sub-vertex to [-g, g], NaN to g, g = twice the guard band
    (DESIGN.md 3, R5)."""
    return xn if xn <= g and xn >= -g else (-g if xn <= g else g)


def _snap(v4, W, H, clamp=None):
    """R1 + R2 in float32: snapped window coordinates (1/256 px) of one clip-space vertex (clamp: (2 gx, 2 gy)
    for a clipped face's sub-vertex)."""
    x, y, w = F32(v4[0]), F32(v4[1]), F32(v4[3])
    iw = F32(1.0) / w
    hw, hh = F32(0.5) * F32(W), F32(0.5) * F32(H)
    xn, yn = x * iw, y * iw
    if clamp is not None:
        xn, yn = _guard_clamp(xn, clamp[0]), _guard_clamp(yn, clamp[1])
    X = int(np.rint(((xn + F32(1.0)) * hw) * F32(256.0)))
    Y = int(np.rint(((yn + F32(1.0)) * hh) * F32(256.0)))
    return X, Y


class Tri:
    """One rasterised (sub-)triangle: integer edge functions E_k(P) = A_k Px + B_k Py + C_k (interior
    positive, P in 1/256 px), its vertices' clip w and their parent barycentric basis.  X, Y (snapped, R2) and
    zw (R1's window depth (z * (1 / w)) * 0.5 + 0.5 in float32) are R4's inputs, kept for tests/forward_exact.py."""

    def __init__(self, verts7, W, H, clamp=None):
        X, Y = zip(*(_snap(p[:4], W, H, clamp) for p in verts7))
        A, B, C = [], [], []
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            A.append(Y[a] - Y[b])
            B.append(X[b] - X[a])
            C.append(X[a] * Y[b] - X[b] * Y[a])
        D = A[0] * X[0] + B[0] * Y[0] + C[0]
        sg = 1 if D > 0 else -1
        self.A, self.B, self.C = [sg * a for a in A], [sg * b for b in B], [sg * c for c in C]
        self.D = sg * D
        self.X, self.Y = list(X), list(Y)
        with np.errstate(all="ignore"):
            self.zw = [(F32(p[2]) * (F32(1.0) / F32(p[3]))) * F32(0.5) + F32(0.5) for p in verts7]
        self.w = [float(p[3]) for p in verts7]
        self.basis = [[float(p[4 + i]) for i in range(3)] for p in verts7]

    def E(self, px, py):
        return [self.A[k] * px + self.B[k] * py + self.C[k] for k in range(3)]

    def covers(self, i, j):
        """R3 at pixel centre (i, j) (window coordinates): E > 0, or E == 0 on a left / top edge."""
        E = self.E(256 * i + 128, 256 * j + 128)
        for k in range(3):
            if E[k] > 0:
                continue
            if E[k] == 0 and (self.A[k] > 0 or (self.A[k] == 0 and self.B[k] < 0)):
                continue
            return False
        return True

    def covers_grid(self, i0, i1, j0, j1):
        """`covers` at every pixel centre of columns i0..i1 and window rows j0..j1 (inclusive): bool [rows, columns]
        and the three edge values there (the same integers: int64 while they fit, Python ints otherwise)."""
        big = max(abs(x) for x in self.A + self.B) * 256 * (max(abs(i0), abs(i1), abs(j0), abs(j1)) + 1) >= 2 ** 61 \
            or max(abs(c) for c in self.C) >= 2 ** 61
        dt = object if big else np.int64
        px = (np.arange(i0, i1 + 1, dtype=np.int64) * 256 + 128).astype(dt)[None, :]
        py = (np.arange(j0, j1 + 1, dtype=np.int64) * 256 + 128).astype(dt)[:, None]
        inside = np.ones((j1 - j0 + 1, i1 - i0 + 1), bool)
        E = []
        for k in range(3):
            e = self.A[k] * px + self.B[k] * py + self.C[k]
            owned = self.A[k] > 0 or (self.A[k] == 0 and self.B[k] < 0)
            inside &= ((e > 0) | ((e == 0) & owned)).astype(bool)
            E.append(e)
        return inside, E

    def weights(self, E2):
        """Parent lambda_i and Wm at the point where the (doubled) edge values are E2 (sum = 2D)."""
        b = [e / (2.0 * self.D) for e in E2]
        q = [b[k] / self.w[k] for k in range(3)]
        sq = q[0] + q[1] + q[2]
        mu = [x / sq for x in q]
        lam = [sum(mu[k] * self.basis[k][i] for k in range(3)) for i in range(3)]
        Wm = sum(mu[k] * self.w[k] for k in range(3))
        return lam, Wm

    def abs_weights(self, E2):
        """The absolute parts of `weights` at the same point: sum_k |b_k / w_k| |basis_ki| (of lambda_i / Wm =
        sum_k (b_k / w_k) basis_ki, the b_k summing to 1) and sum_k |mu_k| |basis_ki| (of lambda_i)."""
        q = [abs(e / (2.0 * self.D)) / self.w[k] for k, e in enumerate(E2)]
        sq = sum(e / (2.0 * self.D) / self.w[k] for k, e in enumerate(E2))
        pair = [sum(q[k] * abs(self.basis[k][i]) for k in range(3)) for i in range(3)]
        col = [sum(q[k] / abs(sq) * abs(self.basis[k][i]) for k in range(3)) for i in range(3)]
        return pair, col


CAP_CULLS = [0]  # faces culled by R5's vertex cap so far (tests)


def _plane(p, v, gx, gy):
    x, y, z, w = v[0], v[1], v[2], v[3]
    return (z + w, gx * w + x, gx * w - x, gy * w + y, gy * w - y)[p]


def setup_face(verts, face, V, W, H):
    """R5: the rasterised triangles of one face ([] = culled) and whether it took the clipping path."""
    if any(not 0 <= int(k) < V for k in face):
        return [], False
    v = [np.asarray(verts[int(k)], F32) for k in face]
    if not all(np.all(np.isfinite(p)) for p in v):
        return [], False
    gx, gy = F32(32768.0) / F32(W), F32(32768.0) / F32(H)
    if all(p[3] > 0 and abs(p[0]) <= gx * p[3] and abs(p[1]) <= gy * p[3] for p in v):
        poly = [np.concatenate([p, np.eye(3, dtype=F32)[k]]) for k, p in enumerate(v)]
        return [Tri(poly, W, H)], False
    poly = [np.concatenate([p, np.eye(3, dtype=F32)[k]]) for k, p in enumerate(v)]
    for pl in range(5):
        out = []
        n = len(poly)
        for i in range(n):
            a, c = poly[i], poly[(i + 1) % n]
            da, dc = _plane(pl, a, gx, gy), _plane(pl, c, gx, gy)
            if (da >= 0) + ((da >= 0) != (dc >= 0)) > 8 - len(out):  # R5 vertex cap: more than 8 culls the face
                CAP_CULLS[0] += 1
                return [], True
            if da >= 0:
                out.append(a)
            if (da >= 0) != (dc >= 0):
                t = da / (da - dc)
                out.append((a + t * (c - a)).astype(F32))
        poly = out
        if len(poly) < 3:
            return [], True
    if not all(p[3] > 0 for p in poly):
        return [], True
    tris = []
    for s in range(len(poly) - 2):
        t3 = [poly[0], poly[s + 1], poly[s + 2]]
        tri = Tri(t3, W, H, (F32(2.0) * gx, F32(2.0) * gy))
        tris.append(tri if tri.D != 0 else None)
    return tris, True


def _record(tris, F, ri):
    """The (sub-)triangle of record index ri: sub-triangle 0 of face f is record f, sub-triangle s > 0 is
    record F + 5 f + s - 1 (the g-buffer's numbering)."""
    if ri < F:
        return ri, tris[ri][0][0]
    d = ri - F
    f = d // EXTRA_PER_FACE
    return f, tris[f][0][d - f * EXTRA_PER_FACE + 1]


def _supported_on(grad_pixels, window):
    """Whether grad_pixels [H,W,C] is zero outside window (i0, i1, j0, j1) (window coordinates, inclusive)."""
    i0, i1, j0, j1 = window
    H = grad_pixels.shape[0]
    return np.count_nonzero(grad_pixels) == np.count_nonzero(grad_pixels[H - 1 - j1:H - j0, i0:i1 + 1])


def backward(vertices, faces, pixels, grad_pixels, gbuffer, track=None, window=None):
    """One frame: vertices [V,4], faces [F,3], pixels / grad_pixels [H,W,C] (rows top first), gbuffer [H,W]
    (visible record, bit 30 = clipped face, -1 background).  Returns float64 (grad_vertices [V,4],
    grad_vertex_colors [V,C], grad_background [H,W,C]).  track: a Bounds to fill next to them (backward_with_bounds).

    window = (i0, i1, j0, j1), window coordinates, inclusive: grad_pixels must be zero outside it (asserted).  Then
    every colour term outside the window and every pair with neither pixel inside it has G = 0 as a factor and is
    exactly zero, so the colour loop visits the window and the pair loop the window and its one-pixel halo, in the
    dense order; pixels are converted one at a time and nothing of the frame's size is allocated.  Returns
    (grad_vertices, grad_vertex_colors, None): grad_background is the cotangent on uncovered pixels, a statement
    about the g-buffer alone.  S, n, N and clip of `track` count the window's terms -- the only non-zero ones."""
    H, W, C = pixels.shape
    V, F = vertices.shape[0], faces.shape[0]
    tris = [setup_face(vertices, faces[f], V, W, H) for f in range(F)]
    gv = np.zeros((V, 4))
    gc = np.zeros((V, C))
    if window is None:
        I = pixels.astype(np.float64)
        G = grad_pixels.astype(np.float64)
        gbg = np.zeros((H, W, C))
        rec = np.where(gbuffer < 0, -1, gbuffer & (GBUF_MULTI - 1))
        ci0, ci1, cj0, cj1 = pi0, pi1, pj0, pj1 = 0, W - 1, 0, H - 1
    else:
        class _PerPixel:  # float64 / the record index of one pixel at a time
            def __init__(self, a, conv):
                self.a, self.conv = a, conv

            def __getitem__(self, rc):
                return self.conv(self.a[rc])
        ci0, ci1, cj0, cj1 = (int(x) for x in window)
        assert 0 <= ci0 <= ci1 < W and 0 <= cj0 <= cj1 < H, window
        assert _supported_on(grad_pixels, (ci0, ci1, cj0, cj1)), "grad_pixels is not zero outside the window"
        I = _PerPixel(pixels, lambda x: x.astype(np.float64))
        G = _PerPixel(grad_pixels, lambda x: x.astype(np.float64))
        gbg = None
        rec = _PerPixel(gbuffer, lambda x: -1 if x < 0 else int(x) & (GBUF_MULTI - 1))
        pi0, pi1, pj0, pj1 = max(ci0 - 1, 0), ci1, max(cj0 - 1, 0), cj1

    def at(i, j):  # window (i, j) -> image row
        return H - 1 - j, i

    def face_covers(f, i, j):
        return any(t is not None and t.covers(i, j) for t in tris[f][0])

    for j in range(cj0, cj1 + 1):
        for i in range(ci0, ci1 + 1):
            r = rec[at(i, j)]
            if r < 0:
                if gbg is not None:
                    gbg[at(i, j)] = G[at(i, j)]
                continue
            f, t = _record(tris, F, int(r))
            lam, _ = t.weights([2 * e for e in t.E(256 * i + 128, 256 * j + 128)])
            for k in range(3):
                gc[faces[f][k]] += lam[k] * G[at(i, j)]
            if track is not None:
                track.colour(faces[f], t, [2 * e for e in t.E(256 * i + 128, 256 * j + 128)], lam, G[at(i, j)],
                             tris[f][1], (i, j))

    def add(ri, i, j, axis, s, omega, s_abs=0.0, own_low=True):
        f, t = _record(tris, F, int(ri))
        if axis == 0:
            E2 = [t.A[k] * (512 * i + 512) + t.B[k] * (512 * j + 256) + 2 * t.C[k] for k in range(3)]
            half, ndc = W / 2.0, (i + 1) / (W / 2.0) - 1.0
        else:
            E2 = [t.A[k] * (512 * i + 256) + t.B[k] * (512 * j + 512) + 2 * t.C[k] for k in range(3)]
            half, ndc = H / 2.0, (j + 1) / (H / 2.0) - 1.0
        lam, Wm = t.weights(E2)
        for k in range(3):
            g = omega * s * half * lam[k] / Wm
            gv[faces[f][k], axis] += g
            gv[faces[f][k], 3] -= g * ndc
        if track is not None:
            track.pair(faces[f], t, E2, axis, omega, s, s_abs, half, ndc, [lam[k] / Wm for k in range(3)], tris[f][1],
                       (i, j), int(ri), own_low)

    for j in range(pj0, pj1 + 1):
        for i in range(pi0, pi1 + 1):
            for axis in (0, 1):
                i2, j2 = (i + 1, j) if axis == 0 else (i, j + 1)
                if i2 >= W or j2 >= H:
                    continue
                rp, rq = int(rec[at(i, j)]), int(rec[at(i2, j2)])
                if rp < 0 and rq < 0:
                    continue
                Ip, Iq = I[at(i, j)], I[at(i2, j2)]
                if (rp < 0 and not np.all(np.isfinite(Ip))) or (rq < 0 and not np.all(np.isfinite(Iq))):
                    continue
                s = -0.5 * float(np.sum((G[at(i, j)] + G[at(i2, j2)]) * (Iq - Ip)))
                if s == 0.0:
                    continue
                sa = 0.0 if track is None else 0.5 * float(np.sum(
                    (np.abs(G[at(i, j)]) + np.abs(G[at(i2, j2)])) * np.abs(Iq - Ip)))
                fp = _record(tris, F, rp)[0] if rp >= 0 else -1
                fq = _record(tris, F, rq)[0] if rq >= 0 else -1
                if fp == fq or fq < 0:
                    add(rp, i, j, axis, s, 1.0, sa)
                elif fp < 0:
                    add(rq, i, j, axis, s, 1.0, sa, False)
                else:
                    p_covers_q, q_covers_p = face_covers(fp, i2, j2), face_covers(fq, i, j)
                    if not p_covers_q and q_covers_p:
                        add(rp, i, j, axis, s, 1.0, sa)
                    elif p_covers_q and not q_covers_p:
                        add(rq, i, j, axis, s, 1.0, sa, False)
                    else:
                        add(rp, i, j, axis, s, 0.5, sa)
                        add(rq, i, j, axis, s, 0.5, sa, False)
    return gv, gc, gbg


def backward_batch(vertices, faces, pixels, grad_pixels, gbuffer, window=None):
    outs = [backward(vertices[b], faces[b], pixels[b], grad_pixels[b], gbuffer[b], None, window)
            for b in range(pixels.shape[0])]
    return tuple(None if outs[0][k] is None else np.stack([o[k] for o in outs]) for k in range(3))


U32 = 2.0 ** -24  # float32's unit roundoff (round to nearest)
INT64_EDGE = 1 << 14  # grad_kernel.h kGradSmallEdge: records with |A_k| or |B_k| from here on take int64 edge values


class Bounds:
    """What `backward` accumulates next to every gradient element for the per-element contract (DESIGN.md 5,
    tests/test_gpu_backward_bound.py):
      S_v [V,4], S_c [V,C]    the sum of the absolute values of the element's terms -- a term with every factor
                              that can cancel replaced by its absolute parts:
                                pair term into dL/dx_i, dL/dy_i   omega S_pair half sum_k |b_k / w_k| |basis_ki|,
                                  S_pair = 0.5 sum_c (|G_c(p)| + |G_c(q)|) |I_c(q) - I_c(p)|,
                                pair term into dL/dw_i            the same times |x_ndc(M)| (|y_ndc(M)|),
                                colour term                       sum_k |mu_k| |basis_ki| |G_c(p)|;
      n_v, n_c                the number of its non-zero terms;
      clip_v [V,4], clip_c [V,C]   whether a clipped (sub-)record contributes to it;
      N_v [V,4]               (column 3 only) sum over the element's terms of omega S_pair half sum_k |b_k / w_k|
                              |basis_ki|: the dL/dx and dL/dy terms whose product with the float32 x_ndc the w
                              component is -- x_ndc = mid (2 / W) - 1 carries an absolute rounding error, not one
                              relative to |x_ndc|;
      L_v [V,4]               sum of E_k(o) |d term / d E_k(o)| over the element's pair terms on records with an edge
                              coefficient |A_k| or |B_k| of at least INT64_EDGE, and of those over the sub-vertices k
                              with |E2_k| < 2 E_k(o) -- o the pixel of the pair that shows the owning record,
                              E2_k = 2 E_k(o) +- one pixel's step: what a rounding of E_k(o) that is relative to
                              E_k(o) costs the element where E_k(o) exceeds half the midpoint value.  Where
                              |E2_k| >= 2 E_k(o) such a rounding is within the same rounding of E2_k and the count
                              of tests/backward_cases.py holds as it stands: nothing is added;
      terms                   (keep_terms) every term as a dict, for tests that rebuild wrong sums from them.
    Pairs the specification skips (a non-finite background on either side, s == 0) add nothing."""

    def __init__(self, V, C, keep_terms=False):
        self.S_v, self.n_v = np.zeros((V, 4)), np.zeros((V, 4), np.int64)
        self.S_c, self.n_c = np.zeros((V, C)), np.zeros((V, C), np.int64)
        self.N_v = np.zeros((V, 4))
        self.L_v = np.zeros((V, 4))
        self.clip_v, self.clip_c = np.zeros((V, 4), bool), np.zeros((V, C), bool)
        self.terms = [] if keep_terms else None
        self.n_half = 0  # pair owners with weight 0.5

    def pair(self, f3, t, E2, axis, omega, s, s_abs, half, ndc, lam_w, clipped, pixel, ri, own_low=True):
        aw, _ = t.abs_weights(E2)
        self.n_half += omega == 0.5
        # E_k at the owner's pixel, exactly: E2_k = 2 E_k(low) + step = 2 E_k(high) - step, step = 256 A_k (256 B_k)
        step = [256 * (t.A[k] if axis == 0 else t.B[k]) for k in range(3)]
        Eo = [(E2[k] - step[k]) // 2 if own_low else (E2[k] + step[k]) // 2 for k in range(3)]
        if max(abs(x) for x in t.A + t.B) >= INT64_EDGE:
            # d term_i / d E_k(o) = omega s half basis_ki / (D w_k) (E2_k / 2D with E2_k = 2 E_k(o) +- step)
            for i in range(3):
                la = omega * s_abs * half * sum(abs(Eo[k]) / (t.D * t.w[k]) * abs(t.basis[k][i]) for k in range(3)
                                                if abs(E2[k]) < 2 * abs(Eo[k]))
                self.L_v[int(f3[i]), axis] += la
                self.L_v[int(f3[i]), 3] += la * abs(ndc)
        for k in range(3):
            v = int(f3[k])
            g, ga = omega * s * half * lam_w[k], omega * s_abs * half * aw[k]
            for col, val, va in ((axis, g, ga), (3, -g * ndc, ga * abs(ndc))):
                self.S_v[v, col] += va
                self.n_v[v, col] += val != 0.0
                self.clip_v[v, col] |= bool(clipped) and val != 0.0
            self.N_v[v, 3] += ga
            if self.terms is not None:
                self.terms.append(dict(kind="pair", vertex=v, axis=axis, pixel=pixel, record=ri, omega=omega, g=g,
                                       ndc=ndc, abs=ga, E2=list(E2), E_owner=Eo, own_low=own_low))

    def colour(self, f3, t, E2, lam, G, clipped, pixel):
        _, ac = t.abs_weights(E2)
        for k in range(3):
            v = int(f3[k])
            val = lam[k] * G
            self.S_c[v] += ac[k] * np.abs(G)
            self.n_c[v] += val != 0.0
            self.clip_c[v] |= bool(clipped) & (val != 0.0)
            if self.terms is not None:
                self.terms.append(dict(kind="colour", vertex=v, pixel=pixel, g=val))


def backward_with_bounds(vertices, faces, pixels, grad_pixels, gbuffer, keep_terms=False, window=None):
    """`backward` (the same values, bit for bit) and the Bounds of its elements."""
    track = Bounds(vertices.shape[0], pixels.shape[2], keep_terms)
    return backward(vertices, faces, pixels, grad_pixels, gbuffer, track, window) + (track,)


def backward_batch_with_bounds(vertices, faces, pixels, grad_pixels, gbuffer, keep_terms=False, window=None):
    """`backward_batch` and one Bounds per frame (window: the same one in every frame; grad_background None)."""
    outs = [backward_with_bounds(vertices[b], faces[b], pixels[b], grad_pixels[b], gbuffer[b], keep_terms, window)
            for b in range(pixels.shape[0])]
    return tuple(None if outs[0][k] is None else np.stack([o[k] for o in outs]) for k in range(3)) + (
        [o[3] for o in outs],)


def stack_bounds(bounds, name):
    """[B, ...] array of one field of a list of Bounds."""
    return np.stack([getattr(b, name) for b in bounds])


def max_rel_err(approx, exact):
    """max |approx - exact| / max |exact| (the gradient's scale)."""
    scale = float(np.max(np.abs(exact))) if exact.size else 0.0
    if scale == 0.0:
        return float(np.max(np.abs(approx))) if approx.size else 0.0
    return float(np.max(np.abs(approx.astype(np.float64) - exact))) / scale

