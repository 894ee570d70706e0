"""The large-frame case table: frames of 4096x4096 to 8192x8192 pinned through windows of the two statements
(tests/forward_exact.py, tests/backward_f64.py, their `window` argument).  TEST INFRASTRUCTURE ONLY.

Shared by tests/test_large_frames.py (the oracle, on a CPU) and tests/test_gpu_large_frames.py (the HIP kernels).

What the frames are there for (dirt_raster.hip make_layout, mirrored by `layout` below):
    4096x4096   64 x 64 = 4096 = kMaxCoarse coarse tiles of 64 px: the last size before the coarse tile grows, and the
                setup's LDS histogram exactly full;
    4097x4097   65 x 65 tiles of 64 px would be 4225, so the coarse tile is 128 px (cshift = 7, 33 x 33 = 1089): the
                first size after growth, with a one-pixel partial coarse tile and a one-pixel partial fine tile in the
                last column and row; one case with C = 7 (specialised channel class), one with C = 5 (generic);
    8192x2049   128 x 33 tiles of 64 px would be 4224: cshift = 7, 64 x 17 = 1088, a partial last row only;
    8192x8192   64 x 64 = 4096 coarse tiles of 128 px and 512 x 512 = 2^18 fine tiles: the size limit, with C = 1
                and C = 3.
Every host array stays under 1 GB (8192 x 8192 x 3 floats are 805 MB).

The scene of a case (`build`), in window pixels: per window a cluster of 12 small perspective faces (vertex offsets
within 8 to 16 px) inside it, a large face (edges of 300 to 3000 px, the int64 edge path) with an edge through it, an
exact depth tie between a small and a large flat face (equal constant zw; their index order alternates from window
to window) and, in the window across a coarse-tile corner, faces whose bounding boxes start at relative coordinates
64 to 127 of a 128-px coarse tile and reach into its right and upper neighbours; then a pair of faces covering the
whole frame and sharing its diagonal, and one face with a vertex beyond the guard band (clipped, several records)
through the frame's centre.

Windows are 48x32 pixels (i0, i1, j0, j1, window coordinates, inclusive): the four corners of the frame, its centre,
a window across the corner of coarse tiles at an odd multiple of 64 in both directions (x = 4032, or 1984 at
W = 8192: a border of 64-px tiles and the middle of a 128-px one), and where the frame has a partial last tile column /
row (4097, 2049) a window on it away from the corners.

CAP (tests/forward_cases.py, 2 % undecided covered pixels) applies per window: a condition on the inputs.
"""
import functools

import numpy as np

import backward_cases as bc
import backward_f64
import forward_cases
import forward_exact
from oracle import oracle

K_MAX_COARSE = 4096   # dirt_raster.hip kMaxCoarse
TILE = 16             # raster_kernel.h kTile
WW, WH = 48, 32       # window size


def layout(W, H):
    """make_layout's coarse-tile arithmetic: (cshift, nctx, ncty, ncoarse, fine tiles)."""
    cshift = 6
    while True:
        nctx, ncty = (W + (1 << cshift) - 1) >> cshift, (H + (1 << cshift) - 1) >> cshift
        if nctx * ncty <= K_MAX_COARSE:
            return cshift, nctx, ncty, nctx * ncty, ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
        cshift += 1


def windows_of(W, H):
    # an odd multiple of 64 in x and in y, more than 640 px from the other windows (the reach of their tie faces)
    bx, by = 4032 if W < 8192 else 1984, 64 * ((5 * H // 8 // 64) | 1)
    w = {
        "corner_00": (0, WW - 1, 0, WH - 1),
        "corner_w0": (W - WW, W - 1, 0, WH - 1),
        "corner_0h": (0, WW - 1, H - WH, H - 1),
        "corner_wh": (W - WW, W - 1, H - WH, H - 1),
        "centre": (W // 2 - WW // 2, W // 2 + WW // 2 - 1, H // 2 - WH // 2, H // 2 + WH // 2 - 1),
        "coarse_corner": (bx - WW // 2, bx + WW // 2 - 1, by - WH // 2, by + WH // 2 - 1),
    }
    if W % TILE:
        w["last_column"] = (W - WW, W - 1, H // 4, H // 4 + WH - 1)
    if H % TILE:
        w["last_row"] = (W // 4, W // 4 + WW - 1, H - WH, H - 1)
    return w


class Case:
    def __init__(self, name, W, H, C, seed, cshift, ncoarse, why):
        self.name, self.W, self.H, self.C, self.seed, self.cshift, self.ncoarse, self.why = (
            name, W, H, C, seed, cshift, ncoarse, why)
        self.windows = windows_of(W, H)

    def __repr__(self):
        return self.name


CASES = [
    Case("4096x4096_c3", 4096, 4096, 3, 1, 6, 4096, "the last size before the coarse tile grows; a full histogram"),
    Case("4097x4097_c7", 4097, 4097, 7, 2, 7, 1089, "first size after growth, partial tiles; specialised C = 7"),
    Case("4097x4097_c5", 4097, 4097, 5, 3, 7, 1089, "first size after growth, partial tiles; generic channel class"),
    Case("8192x2049_c3", 8192, 2049, 3, 4, 7, 1088, "first size after growth in x; a partial last row"),
    Case("8192x8192_c1", 8192, 8192, 1, 5, 7, 4096, "the size limit: 4096 tiles of 128 px, 2^18 fine tiles; C = 1"),
    Case("8192x8192_c3", 8192, 8192, 3, 6, 7, 4096, "the size limit: 4096 tiles of 128 px, 2^18 fine tiles; C = 3"),
]
BY_NAME = {c.name: c for c in CASES}
PAIRS = [(c.name, w) for c in CASES for w in c.windows]  # every (case, window)


def _through(rng, centre, lo, hi):
    """A triangle of edges between about lo and hi px with one edge through `centre` (jittered by 6 px), the
    window lying half inside it; and the point of that edge next to the centre with the normal into the face."""
    th = rng.uniform(0, 2 * np.pi)
    d = np.array([np.cos(th), np.sin(th)])
    n = np.array([-d[1], d[0]])
    c = np.asarray(centre, np.float64) + rng.uniform(-6, 6, 2)
    return [c + rng.uniform(lo, hi) * 0.5 * d, c - rng.uniform(lo, hi) * 0.5 * d, c + rng.uniform(lo, hi) * n], c, n


def build(case):
    """(background [H,W,C], vertices [V,4], colours [V,C], faces [F,3]) of a case: split vertices, float32."""
    if hasattr(case, "build"):
        return case.build()
    W, H, C = case.W, case.H, case.C
    rng = np.random.default_rng(case.seed)
    pts, zs, ws = [], [], []

    def add(tri, z, w=(1.0, 1.0, 1.0)):
        pts.append(np.asarray(tri, np.float64))
        zs.append(np.broadcast_to(np.asarray(z, np.float64), (3,)))
        ws.append(np.asarray(w, np.float64))

    for k, (i0, i1, j0, j1) in enumerate(case.windows.values()):
        mid = np.array([(i0 + i1 + 1) / 2.0, (j0 + j1 + 1) / 2.0])
        for _ in range(12):  # the cluster: small perspective faces inside the window
            c = np.array([rng.uniform(i0 + 4, i1 - 3), rng.uniform(j0 + 4, j1 - 3)])
            ang, rad = rng.uniform(0, 2 * np.pi, 3), rng.uniform(8, 16) * np.sqrt(rng.uniform(0.25, 1, 3))
            add(c + np.stack([np.cos(ang) * rad, np.sin(ang) * rad], 1),
                rng.uniform(-0.9, -0.4) + rng.uniform(-0.01, 0.01, 3), rng.uniform(1, 3, 3))
        add(_through(rng, mid, 300, 3000)[0], rng.uniform(0.0, 0.5, 3))  # a large face crossing the window
        # an exact depth tie behind the cluster, in front of everything else of the window: a small flat face across
        # the edge of a large one of equal zw, in either index order
        large, at, inward = _through(rng, mid, 300, 600)
        small = at + 6.0 * inward + 12.0 * np.array([[1, 0], [-0.5, 0.9], [-0.5, -0.9]])
        for tri in ((small, large) if k % 2 else (large, small)):
            add(tri, -0.25)
    # bounding boxes starting at relative 64..127 of the 128-px coarse tile, reaching into its neighbours
    i0, i1, j0, j1 = case.windows["coarse_corner"]
    tx, ty = (i0 >> 7) << 7, (j0 >> 7) << 7
    for _ in range(4):
        x0, y0 = tx + 64 + rng.uniform(8, 20), ty + 64 + rng.uniform(6, 14)
        x1, y1 = tx + 128 + rng.uniform(5, 60), ty + 128 + rng.uniform(5, 60)
        add([[x0, y0], [x1, y0 + rng.uniform(0, 8)], [x0 + rng.uniform(0, 8), y1]],
            rng.uniform(-0.39, -0.31))  # (behind the cluster)
    # the whole frame, two faces sharing the diagonal, at the back
    add([[0, 0], [W, 0], [W, H]], [0.7, 0.8, 0.9])
    add([[0, 0], [W, H], [0, H]], [0.7, 0.9, 0.8])
    # a vertex beyond the guard band (16384 px from the frame's centre): clipped, several records
    add([[W / 2 - 400, H / 2 + 100], [W / 2 + 100, H / 2 - 400], [W / 2 + 20000, H / 2 + 18000]], [-0.2, -0.15, -0.1])

    p, z, w = np.concatenate(pts), np.concatenate(zs), np.concatenate(ws)
    ndc = p * 2.0 / np.array([W, H], np.float64) - 1.0
    v = (np.concatenate([ndc, z[:, None], np.ones((len(p), 1))], 1) * w[:, None]).astype(np.float32)
    faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    cols = rng.uniform(0, 1, size=(len(v), C)).astype(np.float32)
    bg = rng.random((H, W, C), dtype=np.float32)
    return bg, v, cols, faces


class Bulk:
    """A case's inputs (batched, B = 1) and the oracle's forward: the frame-sized arrays.  One case at a time is
    kept (bulk()); nothing in it is modified."""

    def __init__(self, case):
        self.case = case
        self.inputs = bg, v, c, f = tuple(a[None] for a in build(case))
        self.px, self.gb, self.depth, self.bary, self.face, _ = oracle.rasterise_fwd_gbuffer(bg, v, c, f)
        for a in self.inputs + (self.px, self.gb, self.depth, self.bary, self.face):
            a.setflags(write=False)


@functools.lru_cache(maxsize=1)
def bulk(name):
    return Bulk(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def frame(name, window):
    """The forward statement of one window (small: kept for the whole run), its conditions asserted."""
    case = BY_NAME[name]
    bg, v, c, f = bulk(name).inputs
    fr = forward_exact.Frame(v[0], f[0], case.W, case.H, window=case.windows[window])
    condition(case, window, fr)
    return fr


def condition(case, window, fr):
    """What the case and the window are there for, from the layout arithmetic and the statement."""
    W, H = case.W, case.H
    cshift, nctx, ncty, ncoarse, ntiles = layout(W, H)
    assert (cshift, ncoarse) == (case.cshift, case.ncoarse), (cshift, ncoarse)
    if case.name.startswith("4096x4096"):
        assert ncoarse == K_MAX_COARSE and layout(W + 1, H)[0] == 7
    if case.name.startswith("8192x8192"):
        assert ncoarse == K_MAX_COARSE and ntiles == 1 << 18
    if case.name.startswith(("4097", "8192x2049")):
        assert layout(W - 1, H - 1)[0] == 6  # the first size after growth
    i0, i1, j0, j1 = case.windows[window]
    assert 0 <= i0 and i1 < W and 0 <= j0 and j1 < H and i1 - i0 < 64 and j1 - j0 < 48
    cs = 1 << cshift
    if window.startswith("corner"):
        assert (i0 == 0 or i1 == W - 1) and (j0 == 0 or j1 == H - 1)
        assert (i0 >> cshift == 0 or i1 >> cshift == nctx - 1) and (j0 >> cshift == 0 or j1 >> cshift == ncty - 1)
    if window == "coarse_corner":
        # a 64-px border inside the window in both directions; with 128-px tiles it is no coarse border: the
        # window's upper right part lies at relative coordinates 64 and up of one coarse tile
        bx, by = (i0 + 63) & ~63, (j0 + 63) & ~63
        assert i0 < bx <= i1 and j0 < by <= j1 and bx % 128 == 64 and by % 128 == 64
        assert (i0 >> 6 != i1 >> 6) and (j0 >> 6 != j1 >> 6)
        if cshift == 7:
            assert i0 >> 7 == i1 >> 7 and j0 >> 7 == j1 >> 7 and i1 % cs >= 64 and j1 % cs >= 64
    if window == "last_column":
        assert i1 == W - 1 and W % TILE and (W % cs) < TILE and i0 >> cshift != i1 >> cshift
    if window == "last_row":
        assert j1 == H - 1 and H % TILE and (H % cs) < TILE and j0 >> cshift != j1 >> cshift
    # decided visible records of the window: small ones and ones on the int64 edge path (grad_kernel.h
    # kGradSmallEdge), and -- every window but the guard-band face's -- both kinds
    vis = {int(fr.rec[w[0]]) for row in fr.winners for w in row if len(w) == 1}
    large = {ri for ri in vis if max(abs(x) for x in fr.rec_tri[ri][2].A + fr.rec_tri[ri][2].B) >= bc.SMALL_EDGE}
    assert large and vis - large, (case.name, window, len(vis), len(large))
    if window == "centre":
        assert any(fr.rec_tri[ri][3] for ri in vis), "the clipped face is not visible in the centre window"
    if window == "coarse_corner" and cshift == 7:
        # visible records whose bounding box starts at relative 64..127 of the window's coarse tile and ends past it
        def straddles(t):
            x0, x1 = (min(t.X) + 127) // 256, (max(t.X) - 128) // 256
            y0, y1 = (min(t.Y) + 127) // 256, (max(t.Y) - 128) // 256
            return (x0 >> 7 == i0 >> 7 and x0 % 128 >= 64 and x1 >> 7 > i0 >> 7 and
                    y0 >> 7 == j0 >> 7 and y0 % 128 >= 64 and y1 >> 7 > j0 >> 7)
        assert sum(straddles(fr.rec_tri[ri][2]) for ri in vis) >= 2
    # the exact tie: both flat faces of the window's tie cover a common pixel, and the lower face is the winner
    flat = np.nonzero(fr.flat & fr.certain)[0]
    tie = flat[fr.z[flat] == 0.375]  # (zw of z = -0.25, w = 1: the ties' depth and nothing else's)
    vis = {int(a) for row in fr.winners for w in row if len(w) == 1 for a in w}
    shown = [a for a in tie if int(a) in vis and ((fr.pix[tie] == fr.pix[a]).sum() >= 2)]
    assert shown, "no visible pixel with an exact depth tie"
    for a in shown:
        assert fr.face[a] == fr.face[tie[fr.pix[tie] == fr.pix[a]]].min()


def check_forward(name, window, pixels, gbuffer=None, depth=None, barycentrics=None, face_ids=None, label=""):
    """forward_exact.check_frame on one window of whole-frame outputs ([H,W,...], one frame); prints the figures
    and asserts the cap."""
    b = bulk(name)
    r = forward_exact.check_frame(frame(name, window), b.inputs[0][0], b.inputs[2][0], pixels, gbuffer, depth,
                                  barycentrics, face_ids)
    print("%s %s%s: worst error / (2^-24 sum|terms|): depth %.2f (k = %d), barycentrics %.2f (k = %d), colours %.2f "
          "(k = %d); undecided %d of %d covered pixels" % (
              name, window, label, r["depth"], forward_exact.K_DEPTH, r["barycentrics"], forward_exact.K_BARY,
              r["colours"], forward_exact.K_COLOUR, r["undecided"], r["covered"]))
    assert r["covered"] > 0 and r["share"] <= forward_cases.CAP, "%s %s: %.2f %% of the covered pixels undecided" % (
        name, window, 100.0 * r["share"])
    return r


def cotangent(name, window):
    """grad_pixels [1,H,W,C] supported on the window: standard normal inside, zero outside (fresh, writable)."""
    case = BY_NAME[name]
    i0, i1, j0, j1 = case.windows[window]
    gp = np.zeros((1, case.H, case.W, case.C), np.float32)
    seed = case.seed * 100 + list(case.windows).index(window)
    gp[0, case.H - 1 - j1:case.H - j0, i0:i1 + 1] = np.random.default_rng(seed).standard_normal(
        (j1 - j0 + 1, i1 - i0 + 1, case.C)).astype(np.float32)
    if hasattr(case, "support"):  # (one pixel of the window only)
        i, j = case.support[window]
        keep = gp[0, case.H - 1 - j, i].copy()
        gp[0, case.H - 1 - j1:case.H - j0, i0:i1 + 1] = 0.0
        gp[0, case.H - 1 - j, i] = keep
    return gp


def background_cotangent(name, window, gp, gb):
    """grad_background of the whole frame for a cotangent gp supported on the window: gp where the g-buffer gb is
    -1, else 0.  Zeroes gp's covered pixels in place (inside the window: it is zero elsewhere) and returns it."""
    case = BY_NAME[name]
    i0, i1, j0, j1 = case.windows[window]
    rows, cols = slice(case.H - 1 - j1, case.H - j0), slice(i0, i1 + 1)
    gp[0, rows, cols][np.asarray(gb)[0, rows, cols] >= 0] = 0.0
    return gp


class WindowReference(bc.Reference):
    """backward_cases.Reference for a cotangent supported on one window: the windowed float64 statement and its
    bounds (small: kept for the whole run).  The g-buffer and pixels it reads are the oracle's forward."""

    def __init__(self, name, window, keep_terms=False):
        case = BY_NAME[name]
        b = bulk(name)
        bg, v, c, f = b.inputs
        self.window = case.windows[window]
        gp = cotangent(name, window)
        self.gv, self.gc, self.gbg, self.bounds = backward_f64.backward_batch_with_bounds(
            v, f, b.px, gp, b.gb, keep_terms, window=self.window)
        for n in ("S_v", "n_v", "S_c", "n_c", "N_v", "L_v", "clip_v", "clip_c"):
            setattr(self, n, backward_f64.stack_bounds(self.bounds, n))
        self.C = case.C


@functools.lru_cache(maxsize=None)
def reference(name, window):
    ref = WindowReference(name, window, keep_terms=hasattr(BY_NAME[name], "support"))
    assert ref.n_v.sum() > 0
    if hasattr(BY_NAME[name], "support"):
        BY_NAME[name].condition(window, ref)
    else:
        # vertices that do not reach the window have no terms: their elements must come out exactly zero
        assert ref.n_c.sum() > 0 and (ref.S_v[..., 0] == 0).sum() > ref.S_v.shape[1] // 2
    return ref


class SingleTermCase:
    """`large_edge_single_term` (the int64 edge path of the backward): 8192x8192, C = 3, eight records
    with an edge of 2021 px that runs within 1/256 px of a pixel border -- x = b for four of them, y = b for the
    other four -- and the vertex k opposite it 700 px away; the face on the low side of the border for half of
    them, on the high side for the others; k = 0, 1, 2 by the vertex order.  Nothing else is in the frame.  Per
    record a window of the two pixels on either side of the border (two pixels wide, or high), and a cotangent on
    the pixel the face does NOT cover.  Then the only pair with a non-zero scalar is the one across the edge, owned
    by the record, and each element of its three vertices has exactly one term.  At the covered pixel o,
    E_k(o) = |edge| * (distance from the edge) >= 2^24, and the pair's midpoint lies within 1/256 px of the edge:
    |E2_k| <= E_k(o) / 64.  A rounding of E_k(o) that is relative to E_k(o) is then 64 times and more the same
    rounding of E2_k.  `condition` asserts all of this from the statement's terms."""
    name, W, H, C, seed = "large_edge_single_term", 8192, 8192, 3, 9
    cshift, ncoarse = 7, 4096
    REACH = 700.0 + 13 / 256.0
    #          axis, border b, position r along it, face on the low side, k
    RECORDS = [(0, 1000, 1500, True, 0), (0, 4097, 5000, False, 1), (0, 8000, 2500, True, 2), (0, 6001, 7000, False, 0),
               (1, 1201, 3000, True, 1), (1, 4095, 700, False, 2), (1, 8100, 5500, True, 0), (1, 5003, 7800, False, 1)]

    def __init__(self):
        self.windows, self.support, self.vertex = {}, {}, {}
        for n, (axis, b, r, low, k) in enumerate(self.RECORDS):
            w = "%s_%d_%s_k%d" % ("xy"[axis], b, "low" if low else "high", k)
            lo, hi = ((b - 1, r), (b, r)) if axis == 0 else ((r, b - 1), (r, b))
            self.windows[w] = (lo[0], hi[0], lo[1], hi[1])
            self.support[w] = hi if low else lo
            self.vertex[w] = (3 * n + k, axis, lo if low else hi)

    def __repr__(self):
        return self.name

    def build(self):
        rng = np.random.default_rng(self.seed)
        pts, ws = [], []
        for axis, b, r, low, k in self.RECORDS:
            # along the border from 30 % before r to 70 % after it, crossing it from -1/256 to +1/256 px; odd numbers
            # of 1/256 px, so that the edge values at a pixel centre are not multiples of a high power of two
            e0, e1 = (b - 1 / 256.0, r - 611 - 37 / 256.0), (b + 1 / 256.0, r + 1409 + 200 / 256.0)
            third = (b - self.REACH if low else b + self.REACH, r + 633 + 91 / 256.0)
            tri = [third, e0, e1]
            w = [1.5, 1.0, 1.0]
            tri, w = tri[-k:] + tri[:-k] if k else tri, w[-k:] + w[:-k] if k else w  # (vertex k is the third one)
            pts += [(p if axis == 0 else p[::-1]) for p in tri]
            ws += w
        p, w = np.array(pts, np.float64), np.array(ws, np.float64)
        ndc = p * 2.0 / np.array([self.W, self.H], np.float64) - 1.0
        z = np.repeat(rng.uniform(-0.5, 0.5, len(self.RECORDS)), 3)
        v = (np.concatenate([ndc, z[:, None], np.ones((len(p), 1))], 1) * w[:, None]).astype(np.float32)
        faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
        cols = rng.uniform(0, 1, size=(len(v), self.C)).astype(np.float32)
        bg = rng.random((self.H, self.W, self.C), dtype=np.float32)
        return bg, v, cols, faces

    def condition(self, window, ref):
        vk, axis, owner = self.vertex[window]
        k = vk % 3
        mine = [t for t in ref.bounds[0].terms if t["kind"] == "pair"]
        assert len(mine) == 3 and {t["vertex"] for t in mine} == {vk - k, vk - k + 1, vk - k + 2}, mine
        (t,) = [t for t in mine if t["vertex"] == vk]
        low = self.windows[window][0::2]
        assert t["axis"] == axis and t["omega"] == 1.0 and t["pixel"] == low and t["g"] != 0.0
        assert t["own_low"] == (owner == low) and t["record"] == vk // 3
        assert t["E_owner"][k] >= 1 << 24 and abs(t["E2"][k]) <= t["E_owner"][k] // 64, (t["E_owner"], t["E2"])
        assert ref.n_v[0, vk, axis] == 1 and ref.n_v[0, vk, 3] == 1 and ref.n_c.sum() == 0 and ref.L_v[0, vk, axis] > 0
        assert ref.L_v[0, vk, axis] >= 64 * ref.S_v[0, vk, axis]


SINGLE = SingleTermCase()
BY_NAME[SINGLE.name] = SINGLE
SINGLE_PAIRS = [(SINGLE.name, w) for w in SINGLE.windows]
