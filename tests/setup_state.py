"""Statement, decoder and checker of the setup stage's state.  TEST INFRASTRUCTURE ONLY.

The rasteriser's first stage (setup_kernel, clip_face, make_record and the fused small-scene setup of the raster
kernel) leaves records and FaceData in `saved` and counts, parity words and bin entries in `scratch`.  The rest of
the suite sees that state only through the pixels the later stages make of it; this module reads it directly.

  * decode(): numpy structured views of `saved` / `scratch` bytes at the offsets dirt_debug_layout reports.
  * frame_statement(): what one frame's setup must leave, built from backward_f64.setup_face (R1/R2/R5 in numpy
    float32, R3 on Python integers) and forward_exact's bounding-box and depth-plane rules.  It adds no clipping or
    snapping algebra: only the record slots, the emptiness rule, FaceData, the flag words and the bins.
  * check(): decoded state against statements -> a list of findings, each naming frame, face / record / tile and
    field.  Exact fields are compared for equality (floats bit for bit, NaN matching NaN); za / zb against the exact
    rational plane slope within forward_exact's 6 u (|term 1| + |term 2|) / |det| (times its SLACK).
  * encode(): the statement written into `saved` / `scratch`-shaped byte arrays (tests/test_setup_state_cpu.py
    checks the checker with it).

Left free on purpose: the order of a slab's entries, entries past min(count, slab), every field of an empty record
but `i0 > i1` and `face`, record slots past a face's `nsub`, the second half (iw, basis) of a record of a face that
was not clipped, za / zb of a record with a non-finite zw, the deep-cull words of the flag area and the
neighbour-coverage bits."""
import contextlib
from fractions import Fraction

import numpy as np

import backward_f64
from backward_f64 import EXTRA_PER_FACE
from forward_exact import SLACK, U, record_index

F32 = np.float32

# Field offsets written out once from raster_rules.h (Rec, 128 B; FaceData, 32 B); a bin entry is 8 B
REC = np.dtype({
    "names": ["A", "B", "X0", "Y0", "D", "i0", "i1", "j0", "j1", "z0", "za", "zb", "face", "iw", "basis"],
    "formats": [("<i4", 3), ("<i4", 3), "<i4", "<i4", "<i8", "<u2", "<u2", "<u2", "<u2", "<f4", "<f4", "<f4", "<i4",
                ("<f4", 3), ("<f4", 9)],
    "offsets": [0, 12, 24, 28, 32, 40, 42, 44, 46, 48, 52, 56, 60, 64, 76],
    "itemsize": 128})
FACEDATA = np.dtype({"names": ["v", "q", "nsub", "clipped"], "formats": [("<i4", 3), ("<f4", 3), "<i4", "<i4"],
                     "offsets": [0, 12, 24, 28], "itemsize": 32})
ENTRY = np.dtype([("ri", "<u4"), ("rel", "<u4")])
FLAG_WORDS = 64  # the 256-B flag area

MAX_FINDINGS = 40  # per check(): a broken stage would otherwise report every record


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def same_f32(a, b):
    """Bit-for-bit equality of float32 values; a NaN matches any NaN (payloads are not part of the statement)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------ decoder


class Decoded:
    """Views of one `saved` / `scratch` pair: recs [B, 6F], fdata [B, F], counts [2, B, ncoarse] (the strided
    counters), flag [64], bins [B, ncoarse, slab].  The views alias the byte arrays (a mutation shows)."""

    def __init__(self, L, B, F, saved, scratch):
        assert REC.itemsize == L["sizeof_Rec"] and FACEDATA.itemsize == L["sizeof_FaceData"], "record sizes"
        assert REC.fields["i0"][1] == L["kRecBboxOffset"], "bbox offset"
        assert ENTRY.itemsize == 8
        self.L, self.B, self.F = L, B, F
        nrec, nc, slab, stride = L["nrec"], L["nctx"] * L["ncty"], L["slab"], L["kCountStride"]
        assert nrec == (1 + EXTRA_PER_FACE) * F
        self.ncoarse = nc
        saved, scratch = np.asarray(saved, np.uint8), np.asarray(scratch, np.uint8)
        # (the neighbour-coverage bits that end `saved` are not looked at and need not be passed)
        assert saved.size >= L["saved_cov"] and scratch.size >= L["scratch_total"]
        self.recs = saved[:B * nrec * REC.itemsize].view(REC).reshape(B, nrec)
        o = L["saved_fdata"]
        self.fdata = saved[o:o + B * F * FACEDATA.itemsize].view(FACEDATA).reshape(B, F)
        o = L["off_count"]
        words = scratch[o:o + 2 * B * nc * stride * 4].view("<u4")
        self.counts = words.reshape(2, B, nc, stride)[..., 0]
        o = L["off_flag"]
        self.flag = scratch[o:o + 4 * FLAG_WORDS].view("<u4")
        o = L["off_bins"]
        self.bins = scratch[o:o + B * nc * slab * 8].view(ENTRY).reshape(B, nc, slab)


def decode(L, B, F, saved, scratch):
    return Decoded(L, B, F, saved, scratch)


# ---------------------------------------------------------------------------------------------- statement


@contextlib.contextmanager
def _watch_clamp():
    """Whether the statement's own R5 sub-vertex clamp (backward_f64._guard_clamp) moved a coordinate."""
    moved = [False]
    orig = backward_f64._guard_clamp

    def watched(xn, g):
        r = orig(xn, g)
        if not r == xn:
            moved[0] = True
        return r

    backward_f64._guard_clamp = watched
    try:
        yield moved
    finally:
        backward_f64._guard_clamp = orig


class RecordStatement:
    """One specified record slot: `tri` None or `bbox` None = empty."""

    def __init__(self, ri, f, s, tri, clipped, W, H):
        self.ri, self.f, self.s, self.tri, self.clipped = ri, f, s, tri, clipped
        self.bbox = None
        if tri is not None and tri.D != 0:
            # forward_exact.Frame._add_record's box, clamped to the frame
            i0, i1 = max(0, (min(tri.X) - 128 + 255) // 256), min(W - 1, (max(tri.X) - 128) // 256)
            j0, j1 = max(0, (min(tri.Y) - 128 + 255) // 256), min(H - 1, (max(tri.Y) - 128) // 256)
            if i0 <= i1 and j0 <= j1:
                self.bbox = (i0, i1, j0, j1)

    @property
    def empty(self):
        return self.bbox is None

    def plane(self):
        """((za, bound), (zb, bound)) as Fractions: the exact slopes of the plane through (X, Y, zw) and
        forward_exact's 6 u (|term 1| + |term 2|) / |det| SLACK; None when a zw is not finite; "flat" when the
        three zw are equal (za = zb = 0 exactly)."""
        t = self.tri
        zw = [float(z) for z in t.zw]
        if not all(np.isfinite(z) for z in zw):
            return None
        if zw[0] == zw[1] == zw[2]:
            return "flat"
        z = [Fraction(v) for v in zw]
        dz1, dz2 = z[1] - z[0], z[2] - z[0]
        dx1, dy1 = Fraction(t.X[1] - t.X[0], 256), Fraction(t.Y[1] - t.Y[0], 256)
        dx2, dy2 = Fraction(t.X[2] - t.X[0], 256), Fraction(t.Y[2] - t.Y[0], 256)
        det = dx1 * dy2 - dx2 * dy1  # signed: the vertices' own orientation, = +-D / 65536
        assert abs(det) == Fraction(t.D, 65536)
        k = 6 * Fraction(U) * Fraction(SLACK) / abs(det)
        a1, a2, b1, b2 = dz1 * dy2, dz2 * dy1, dx1 * dz2, dx2 * dz1
        return ((a1 - a2) / det, k * (abs(a1) + abs(a2))), ((b1 - b2) / det, k * (abs(b1) + abs(b2)))


class FrameStatement:
    """What the setup of one frame (vertices [V, 4], faces [F, 3], W x H pixels) must leave.

    faces: per face (v raw indices, q float32 [3], nsub, clipped); records: {record index: RecordStatement} for the
    specified slots (slot f always, slots of sub-triangles 1 .. nsub - 1); oob: some index outside [0, V);
    cap_culled / clamped: the frame's R5 deviation counts."""

    def __init__(self, vertices, faces, W, H):
        vertices, faces = np.asarray(vertices, F32), np.asarray(faces)
        self.W, self.H, self.V, self.F = W, H, vertices.shape[0], faces.shape[0]
        V, F = self.V, self.F
        self.faces, self.records = [], {}
        self.oob, self.cap_culled, self.clamped = False, 0, 0
        for f in range(F):
            idx = [int(k) for k in faces[f]]
            inr = [0 <= k < V for k in idx]
            self.oob = self.oob or not all(inr)
            cap0 = backward_f64.CAP_CULLS[0]
            with _watch_clamp() as moved, np.errstate(all="ignore"):
                subs, clipped = backward_f64.setup_face(vertices, faces[f], V, W, H)
            self.cap_culled += backward_f64.CAP_CULLS[0] - cap0
            self.clamped += 1 if (clipped and moved[0]) else 0
            w = [vertices[k][3] if ok else F32(1.0) for k, ok in zip(idx, inr)]
            if subs and not clipped:
                with np.errstate(all="ignore"):
                    q = [F32(1.0) / F32(x) for x in w]
            else:
                q = w
            self.faces.append((idx, np.array(q, F32), len(subs), bool(clipped)))
            self.records[f] = RecordStatement(f, f, 0, subs[0] if subs else None, clipped, W, H)
            for s in range(1, len(subs)):
                ri = record_index(F, f, s)
                self.records[ri] = RecordStatement(ri, f, s, subs[s], clipped, W, H)
        self._tiles = {}

    def tiles(self, cshift):
        """{coarse tile index: {record index: rel_bbox}} for coarse tiles of edge 1 << cshift: every non-empty
        record whose bbox meets the tile, with its bbox relative to the tile's origin and clamped to it."""
        if cshift not in self._tiles:
            nctx = (self.W + (1 << cshift) - 1) >> cshift
            lim = (1 << cshift) - 1
            out = {}
            for ri, r in self.records.items():
                if r.empty:
                    continue
                i0, i1, j0, j1 = r.bbox
                for cy in range(j0 >> cshift, (j1 >> cshift) + 1):
                    for cx in range(i0 >> cshift, (i1 >> cshift) + 1):
                        ox, oy = cx << cshift, cy << cshift
                        rel = (max(i0 - ox, 0) | min(i1 - ox, lim) << 8 | max(j0 - oy, 0) << 16
                               | min(j1 - oy, lim) << 24)
                        out.setdefault(cy * nctx + cx, {})[ri] = rel
            self._tiles[cshift] = out
        return self._tiles[cshift]

    def coarse_tiles_of(self, ri, cshift):
        r = self.records[ri]
        if r.empty:
            return 0
        i0, i1, j0, j1 = r.bbox
        return ((i1 >> cshift) - (i0 >> cshift) + 1) * ((j1 >> cshift) - (j0 >> cshift) + 1)


def frame_statement(vertices, faces, W, H):
    return FrameStatement(vertices, faces, W, H)


class Expect:
    """What check() holds a decoded state to: the B frames' statements (one object may stand for identical frames)
    and the scratch's history since it was zeroed -- `binned`: the number of binned forwards (0: only fused ones, the
    counts and parity words still zero and the bins not looked at; the last one is the one the statements describe);
    `oob`, `cap_culled`, `clamped`: the flag words (None: the statements' own sums, right after one forward on a
    zeroed scratch; cumulative over the forwards of a DIRT_FWD_SCRATCH_CLEAN sequence); `parity`: (P, Q) where they
    are not the ones `binned` forwards on a zeroed scratch leave."""

    def __init__(self, stmts, binned=1, oob=None, cap_culled=None, clamped=None, parity=None):
        self.stmts, self.binned = list(stmts), binned
        k = binned
        self.parity = (((k - 1) & 1, k & 1) if k > 0 else (0, 0)) if parity is None else tuple(parity)
        self.oob = any(s.oob for s in self.stmts) if oob is None else oob
        self.cap_culled = sum(s.cap_culled for s in self.stmts) if cap_culled is None else cap_culled
        self.clamped = sum(s.clamped for s in self.stmts) if clamped is None else clamped


# ------------------------------------------------------------------------------------------------ checker


class _Findings(list):
    def __init__(self):
        super().__init__()
        self.total = 0
        self.worst_plane = 0.0  # worst |za or zb - exact| / bound seen

    def add(self, msg):
        self.total += 1
        if len(self) < MAX_FINDINGS:
            self.append(msg)


def _check_record(out, b, rs, rec):
    where = "frame %d record %d (face %d sub %d)" % (b, rs.ri, rs.f, rs.s)
    if rs.empty:
        if not int(rec["i0"]) > int(rec["i1"]):
            out.add("%s: empty in the statement, but i0 = %d <= i1 = %d" % (where, rec["i0"], rec["i1"]))
        if int(rec["face"]) != rs.f:
            out.add("%s: face = %d on an empty record" % (where, rec["face"]))
        return
    t = rs.tri
    for name, want in (("A", t.A), ("B", t.B)):
        if [int(x) for x in rec[name]] != list(want):
            out.add("%s: %s = %s, statement %s" % (where, name, rec[name].tolist(), list(want)))
    for name, want in (("X0", t.X[0]), ("Y0", t.Y[0]), ("D", t.D), ("i0", rs.bbox[0]), ("i1", rs.bbox[1]),
                       ("j0", rs.bbox[2]), ("j1", rs.bbox[3]), ("face", rs.f)):
        if int(rec[name]) != want:
            out.add("%s: %s = %d, statement %d" % (where, name, rec[name], want))
    if not int(rec["D"]) > 0:
        out.add("%s: D = %d is not positive" % (where, rec["D"]))
    if not same_f32(rec["z0"], t.zw[0]):
        out.add("%s: z0 = %r, statement zw[0] = %r" % (where, float(rec["z0"]), float(t.zw[0])))
    plane = rs.plane()
    if plane == "flat":
        for name in ("za", "zb"):
            if not float(rec[name]) == 0.0:
                out.add("%s: %s = %r on a flat record (three equal zw)" % (where, name, float(rec[name])))
    elif plane is not None:
        for name, (exact, bound) in zip(("za", "zb"), plane):
            got = float(rec[name])
            if not np.isfinite(got):
                out.add("%s: %s = %r, exact slope %r" % (where, name, got, float(exact)))
                continue
            err = abs(Fraction(got) - exact)
            if bound > 0:
                out.worst_plane = max(out.worst_plane, float(err / bound))
            if err > bound:
                out.add("%s: %s = %r, exact slope %r: error %.3g exceeds the bound %.3g (%.2f of it)"
                        % (where, name, got, float(exact), float(err), float(bound),
                           float(err / bound) if bound > 0 else float("inf")))
    if rs.clipped:
        with np.errstate(all="ignore"):
            iw = np.array([F32(1.0) / F32(w) for w in t.w], F32)
        if not same_f32(rec["iw"], iw):
            out.add("%s: iw = %s, statement 1 / w = %s" % (where, rec["iw"].tolist(), iw.tolist()))
        basis = np.array(t.basis, F32).reshape(9)
        if not same_f32(rec["basis"], basis):
            out.add("%s: basis = %s, statement %s" % (where, rec["basis"].tolist(), basis.tolist()))


def _check_tile(out, b, c, want, n, entries, slab):
    where = "frame %d tile %d" % (b, c)
    m = min(n, slab)
    seen = {}
    for k in range(m):
        ri, rel = int(entries["ri"][k]), int(entries["rel"][k])
        if ri in seen:
            out.add("%s: record %d entered twice (slab positions %d and %d)" % (where, ri, seen[ri], k))
            continue
        seen[ri] = k
        if ri not in want:
            out.add("%s: slab position %d holds record %d, which does not touch the tile (or is empty, stale or "
                    "no record)" % (where, k, ri))
        elif rel != want[ri]:
            out.add("%s: record %d has rel_bbox %#010x, statement %#010x" % (where, ri, rel, want[ri]))
    if n <= slab:
        for ri in sorted(set(want) - set(seen)):
            out.add("%s: record %d is missing from the slab" % (where, ri))


def check(dec, expect):
    """Findings (strings; empty = the state is the statement's).  `.total` counts them all (the list is capped),
    `.worst_plane` is the worst za / zb error as a fraction of its bound."""
    out = _Findings()
    L, B, F = dec.L, dec.B, dec.F
    assert len(expect.stmts) == B
    cshift, slab, nc = L["cshift"], L["slab"], dec.ncoarse
    # flag area
    flag = dec.flag
    if (int(flag[0]) != 0) != bool(expect.oob):
        out.add("flag word 0 = %d, statement: %s face index out of range" % (flag[0], "a" if expect.oob else "no"))
    for name, word, want in (("cap-culled", L["kStatCapCulled"], expect.cap_culled),
                             ("clamped", L["kStatClamped"], expect.clamped)):
        if int(flag[word]) != want:
            out.add("flag word %d (R5 %s faces) = %d, statement %d" % (word, name, flag[word], want))
    k = expect.binned
    P, Q = expect.parity
    if int(flag[L["kParP"]]) != P or int(flag[L["kParQ"]]) != Q:
        out.add("parity words P = %d, Q = %d, statement P = %d, Q = %d after %d binned forwards"
                % (flag[L["kParP"]], flag[L["kParQ"]], P, Q, k))
    checked = {}
    for b, st in enumerate(expect.stmts):
        assert st.F == F
        # FaceData
        for f, (idx, q, nsub, clipped) in enumerate(st.faces):
            fd = dec.fdata[b, f]
            where = "frame %d face %d" % (b, f)
            if [int(x) for x in fd["v"]] != idx:
                out.add("%s: v = %s, statement %s" % (where, fd["v"].tolist(), idx))
            if int(fd["nsub"]) != nsub:
                out.add("%s: nsub = %d, statement %d" % (where, fd["nsub"], nsub))
            if int(fd["clipped"]) != int(clipped):
                out.add("%s: clipped = %d, statement %d" % (where, fd["clipped"], int(clipped)))
            if not same_f32(fd["q"], q):
                out.add("%s: q = %s, statement %s (%s)" % (where, fd["q"].tolist(), q.tolist(),
                                                          "1 / w" if nsub and not clipped else "clip w"))
        # records (identical frames with identical bytes are checked once)
        key = (id(st), dec.recs[b].tobytes())
        if key not in checked:
            checked[key] = b
            for ri, rs in st.records.items():
                _check_record(out, b, rs, dec.recs[b, ri])
        # counts and bins
        tiles = st.tiles(cshift) if k > 0 else {}
        for c in range(nc):
            want = tiles.get(c, {})
            cur, idle = int(dec.counts[P, b, c]), int(dec.counts[P ^ 1, b, c])
            if idle != 0:
                out.add("frame %d tile %d: idle count set %d holds %d" % (b, c, P ^ 1, idle))
            if cur != len(want):
                out.add("frame %d tile %d: count = %d, statement %d" % (b, c, cur, len(want)))
            if k > 0 and cur + idle > 0:
                _check_tile(out, b, c, want, cur + idle, dec.bins[b, c], slab)
    return out


# ------------------------------------------------------------------------------------------------ encoder


def _round_f32(x):
    return F32(float(x))  # (a Fraction rounds to float64, then float32: well inside any bound used here)


def encode(L, B, F, expect, rng=None):
    """`saved` / `scratch` byte arrays holding exactly what `expect` states (entries of each slab in a random order
    when rng is given; an overflowing tile keeps the first `slab` of them)."""
    saved = np.zeros(L["saved_total"], np.uint8)
    scratch = np.zeros(L["scratch_total"], np.uint8)
    dec = Decoded(L, B, F, saved, scratch)
    k = expect.binned
    P, Q = expect.parity
    dec.flag[0] = 1 if expect.oob else 0
    dec.flag[L["kStatCapCulled"]], dec.flag[L["kStatClamped"]] = expect.cap_culled, expect.clamped
    dec.flag[L["kParP"]], dec.flag[L["kParQ"]] = P, Q
    for b, st in enumerate(expect.stmts):
        for f, (idx, q, nsub, clipped) in enumerate(st.faces):
            fd = dec.fdata[b, f]
            fd["v"], fd["q"], fd["nsub"], fd["clipped"] = idx, q, nsub, int(clipped)
        for ri, rs in st.records.items():
            rec = dec.recs[b, ri]
            rec["face"] = rs.f
            if rs.empty:
                rec["i0"], rec["i1"], rec["j0"], rec["j1"] = 1, 0, 1, 0
                continue
            t = rs.tri
            rec["A"], rec["B"], rec["X0"], rec["Y0"], rec["D"] = t.A, t.B, t.X[0], t.Y[0], t.D
            rec["i0"], rec["i1"], rec["j0"], rec["j1"] = rs.bbox
            rec["z0"] = t.zw[0]
            plane = rs.plane()
            if plane is not None and plane != "flat":
                rec["za"], rec["zb"] = _round_f32(plane[0][0]), _round_f32(plane[1][0])
            if rs.clipped:
                with np.errstate(all="ignore"):
                    rec["iw"] = [F32(1.0) / F32(w) for w in t.w]
                rec["basis"] = np.array(t.basis, F32).reshape(9)
        if k > 0:
            for c, want in st.tiles(L["cshift"]).items():
                dec.counts[P, b, c] = len(want)
                items = sorted(want.items())
                if rng is not None:
                    items = [items[i] for i in rng.permutation(len(items))]
                for pos, (ri, rel) in enumerate(items[:L["slab"]]):
                    dec.bins[b, c, pos] = (ri, rel)
    return saved, scratch
