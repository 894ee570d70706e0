"""GPU: the setup stage's records, FaceData, counts, parity words and bin entries read back from `saved` and
`scratch` and held to tests/setup_state.py's statement.

Every case goes through the raw C ABI with caller-owned, zeroed `saved` / `scratch` (dirt_rasterise_fwd at C = 1),
copies both back and runs setup_state.check on them: exact fields by equality, za / zb within forward_exact's bound
(each test prints its worst error as a fraction of that bound).  Each case asserts, from dirt_debug_layout's numbers
and the statement, that it takes the path it is there for: fused or binned, the 128- or 256-thread setup, the
big-record queue and its overflow, slab overflow, cshift = 7."""
import numpy as np
import pytest
import torch

import scenes
import setup_state as ss
from test_gpu_parity import _gpu

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _batched(v, f):
    return (v, f) if v.ndim == 3 else (v[None], f[None])


class _Workspace:
    """Zeroed `saved` and `scratch` of one layout and the forwards run on them."""

    def __init__(self, B, H, W, V, F, bin_capacity=0):
        from dirt_amd import _lib
        self.B, self.H, self.W, self.V, self.F, self.cap = B, H, W, V, F, bin_capacity
        self.L = _lib.debug_layout(B, H, W, F, bin_capacity)
        self.saved_bytes, self.scratch_bytes = _lib.workspace_sizes(B, H, W, 1, V, F, bin_capacity)
        assert (self.saved_bytes, self.scratch_bytes) == (self.L["saved_total"], self.L["scratch_total"])
        self.saved = torch.zeros(self.saved_bytes, dtype=torch.uint8, device="cuda")
        self.scratch = torch.zeros(self.scratch_bytes, dtype=torch.uint8, device="cuda")
        self.bg = torch.zeros((B, H, W, 1), device="cuda")
        self.cols = torch.ones((B, V, 1), device="cuda")
        self.pixels = torch.empty((B, H, W, 1), device="cuda")
        self.gbuffer = torch.empty((B, H, W), dtype=torch.int32, device="cuda")

    # which path a forward of this layout takes, from the accessor's numbers
    @property
    def fused(self):
        L, ntiles = self.L, ((self.W + 15) // 16) * ((self.H + 15) // 16)
        return 0 < self.F <= L["kFusedMaxF"] and self.B * ntiles <= L["kFusedMaxTiles"]

    @property
    def setup_threads(self):
        L = self.L
        small = self.B * ((self.F + L["kBinThreads"] - 1) // L["kBinThreads"]) < L["kSetupSmallGrid"]
        return L["kBinThreads"] // 2 if small else L["kBinThreads"]

    def forward(self, v, f, flags=0):
        from dirt_amd import _lib
        assert v.shape == (self.B, self.V, 4) and f.shape == (self.B, self.F, 3)
        vt, ft = _gpu(v), _gpu(f)
        _lib.check(_lib.load().dirt_rasterise_fwd(
            self.bg.data_ptr(), vt.data_ptr(), self.cols.data_ptr(), ft.data_ptr(), None, self.B, self.H, self.W, 1,
            self.V, self.F, 0, self.pixels.data_ptr(), self.gbuffer.data_ptr(), self.saved.data_ptr(),
            self.saved_bytes, self.scratch.data_ptr(), self.scratch_bytes, self.cap, flags, None, None, _stream()))
        torch.cuda.synchronize()

    def decoded(self):
        torch.cuda.synchronize()
        saved = self.saved[:self.L["saved_cov"]].cpu().numpy()  # (records and FaceData; not the coverage bits)
        return ss.decode(self.L, self.B, self.F, saved, self.scratch.cpu().numpy())


def _statements(v, f, W, H):
    """One statement per frame; frames with the same bytes share one."""
    made, out = {}, []
    for b in range(v.shape[0]):
        key = (v[b].tobytes(), f[b].tobytes())
        if key not in made:
            made[key] = ss.frame_statement(v[b], f[b], W, H)
        out.append(made[key])
    return out


def _assert_clean(found, what):
    print("%s: worst za / zb error %.3f of the bound" % (what, found.worst_plane))
    assert not found, "%d findings, the first ones:\n%s" % (found.total, "\n".join(found))


def _run(v, f, W, H, bin_capacity=0, what="", stmts=None):
    """One forward on a zeroed workspace, checked; returns (workspace, statements, decoded state)."""
    v, f = _batched(v, f)
    ws = _Workspace(v.shape[0], H, W, v.shape[1], f.shape[1], bin_capacity)
    ws.forward(v, f)
    stmts = stmts or _statements(v, f, W, H)
    dec = ws.decoded()
    _assert_clean(ss.check(dec, ss.Expect(stmts, binned=0 if ws.fused else 1)), what)
    return ws, stmts, dec


def _px(tris, W, H, z=0.25):
    """Triangles given in window pixels ([F, 3, 2]) as split clip-space vertices (w = 1) and faces."""
    t = np.asarray(tris, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), t.shape[:2]) if np.ndim(z) else np.full(t.shape[:2], z)
    v = np.stack([t[..., 0] * 2.0 / W - 1.0, t[..., 1] * 2.0 / H - 1.0, z, np.ones(t.shape[:2])], -1)
    return v.reshape(-1, 4).astype(np.float32), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)


# ---- frames and face counts: the 128-thread setup, binned


@pytest.mark.parametrize("H,W,F", [(64, 64, 33), (63, 65, 127), (63, 65, 128), (136, 200, 129), (24, 8192, 300)])
def test_frames_and_face_counts(H, W, F):
    _, v, _, f = scenes.random_triangles(F=F, W=W, H=H, C=1, radius_px=40.0 if W == 8192 else 12.0, seed=H + F)
    ws, stmts, dec = _run(v, f, W, H, what="%dx%d F=%d" % (W, H, F))
    L = ws.L
    assert not ws.fused and ws.setup_threads == 128 and L["cshift"] == 6
    grids = {(64, 64): (1, 1), (63, 65): (2, 1), (136, 200): (4, 3), (24, 8192): (128, 1)}
    assert (L["nctx"], L["ncty"]) == grids[H, W]
    tiles = stmts[0].tiles(6)
    assert len(tiles) > L["nctx"] * L["ncty"] // 2 and max(len(t) for t in tiles.values()) <= L["slab"]
    # around the workgroup edge: one workgroup one face short, a full one, and a second one of a single face
    nwg = (F + ws.setup_threads - 1) // ws.setup_threads
    assert nwg == {33: 1, 127: 1, 128: 1, 129: 2, 300: 3}[F]


def test_cshift_7_frame():
    """8192 x 2112: 128 x 33 tiles of 64 px exceed the 4096 the setup's histogram holds, so coarse tiles are 128 px.
    A handful of faces: one across a 128-px boundary, one across a 64-px boundary that is none at 128, one in the last
    (partial) tile row and column, one spanning several tiles both ways."""
    W, H = 8192, 2112
    tris = [[(120.3, 40.2), (135.7, 44.1), (126.2, 60.9)],        # crosses x = 128
            [(60.2, 185.4), (70.6, 188.3), (64.1, 200.8)],        # crosses x = 64 and y = 192 only: one tile
            [(8180.5, 2100.5), (8191.4, 2101.2), (8185.3, 2111.6)],
            [(1000.2, 100.7), (1700.9, 380.2), (1100.4, 600.3)],
            [(4090.0, 1020.0), (4100.0, 1020.0), (4095.0, 1030.0)],
            [(300.5, 127.9), (310.5, 127.2), (305.5, 128.6)]]     # crosses y = 128 by less than a pixel
    v, f = _px(tris, W, H, z=[[0.1, 0.2, 0.3]] * len(tris))
    ws, stmts, dec = _run(v, f, W, H, what="8192x2112")
    L = ws.L
    assert (L["cshift"], L["nctx"], L["ncty"]) == (7, 64, 17)
    assert ws.F <= L["kFusedMaxF"] and not ws.fused  # binned by the tile count alone
    st = stmts[0]
    assert [st.coarse_tiles_of(ri, 7) for ri in range(3)] == [2, 1, 1] and st.coarse_tiles_of(1, 6) == 4
    assert st.coarse_tiles_of(3, 7) > L["kSmallPairs"]
    assert 64 * 16 + 63 in st.tiles(7)  # the last tile


@pytest.mark.parametrize("F", [40, 255, 256, 257])
def test_256_thread_setup(F):
    """B x ceil(F / 256) reaches kSetupSmallGrid: the 256-thread variant, two geometries alternating over 128
    frames (F 255 / 256 / 257: a workgroup one face short, full, and a second workgroup of one face)."""
    W = H = 64
    B = 128
    a = scenes.random_triangles(F=F, W=W, H=H, C=1, radius_px=10.0, seed=F)
    b = scenes.random_triangles(F=F, W=W, H=H, C=1, radius_px=5.0, seed=F + 1)
    v = np.stack([(a, b)[k % 2][1] for k in range(B)])
    f = np.stack([(a, b)[k % 2][3] for k in range(B)])
    ws, stmts, dec = _run(v, f, W, H, what="B=128 F=%d" % F)
    assert not ws.fused and ws.setup_threads == 256
    assert stmts[0] is stmts[2] and stmts[0] is not stmts[1]


# ---- the big-record queue, one workgroup


def test_big_record_queue():
    """8192 x 24 (128 x 1 coarse tiles), one 128-thread workgroup: records over exactly kSmallPairs tiles (inline) and
    kSmallPairs + 1 (queued), more than kBigCap queued records in consecutive face slots (the rest fall back to the
    inline path), small records in between and one full-frame triangle."""
    W, H = 8192, 24
    rng = np.random.default_rng(7)
    tris = []

    def wide(first_tile, ntiles):
        x0, x1 = 64 * first_tile + 10.3, 64 * (first_tile + ntiles - 1) + 50.6
        return [(x0, 2.2), (x1, 3.1), (0.5 * (x0 + x1), 21.7)]

    tris.append(wide(3, 8))
    tris.append(wide(20, 9))
    for k in range(70):
        tris.append(wide(int(rng.integers(0, 100)), int(rng.integers(9, 28))))
    for k in range(20):
        x, y = rng.uniform(10, W - 10), rng.uniform(5, H - 5)
        tris.append([(x - 4, y - 3), (x + 5, y - 2), (x, y + 4)])
    tris.append([(-10.0, -10.0), (2.4 * W, -10.0), (-10.0, 3 * H)])  # covers the whole frame, inside the guard band
    v, f = _px(tris, W, H, z=rng.uniform(-0.5, 0.5, (len(tris), 3)))
    ws, stmts, dec = _run(v, f, W, H, what="big-record queue")
    L, st = ws.L, stmts[0]
    assert not ws.fused and ws.setup_threads == 128 and ws.F <= 128  # one workgroup, one queue
    n = [st.coarse_tiles_of(ri, 6) for ri in range(ws.F)]
    assert n[0] == L["kSmallPairs"] and n[1] == L["kSmallPairs"] + 1 and n[-1] == 128
    assert all(x > L["kSmallPairs"] for x in n[1:72]) and sum(x > L["kSmallPairs"] for x in n) > L["kBigCap"]
    assert st.records[ws.F - 1].bbox == (0, W - 1, 0, H - 1) and not st.faces[ws.F - 1][3]


# ---- edge faces


def _edge_scene(W, H):
    """Ordinary faces plus one of each edge kind; returns vertices, faces and the face index of each kind."""
    _, v, _, f = scenes.random_triangles(F=40, W=W, H=H, C=1, radius_px=9.0, seed=2, perspective=True)
    v, f, kinds = [v], [f], {}
    nv = [len(v[0])]

    def add(name, verts, face=None):
        verts = np.asarray(verts, np.float32).reshape(-1, 4)
        kinds[name] = sum(len(x) for x in f)
        f.append(np.asarray([face if face is not None else [nv[0], nv[0] + 1, nv[0] + 2]], np.int32))
        v.append(verts)
        nv[0] += len(verts)

    def ndc(x, y, z=0.1, w=1.0):
        return [(x * 2.0 / W - 1.0) * w, (y * 2.0 / H - 1.0) * w, z * w, w]

    add("zero_area", [ndc(10, 10), ndc(20, 20), ndc(30, 30)])
    add("repeated_vertex", [ndc(10, 10), ndc(30, 12)], face=[nv[0], nv[0], nv[0] + 1])
    add("sliver_between_centres", [ndc(5.6, 3.0), ndc(5.9, 3.0), ndc(5.75, 40.0)])  # no pixel centre column inside
    add("row_sliver", [ndc(3.0, 7.55), ndc(50.0, 7.7), ndc(3.0, 7.9)])
    add("off_frame_in_guard_band", [ndc(W + 300.0, 10.0), ndc(W + 340.0, 12.0), ndc(W + 320.0, 50.0)])
    add("below_frame", [ndc(10.0, -500.0), ndc(40.0, -480.0), ndc(20.0, -450.0)])
    add("index_out_of_range", [ndc(10, 10)], face=[nv[0], 0, 10 ** 6])
    add("index_negative", [ndc(10, 10, w=2.5)], face=[-1, nv[0], 1])
    add("index_equals_V", [], face=[0, 1, -7])  # (patched to V below)
    add("nan_vertex", [ndc(10, 10), [np.nan, 0.2, 0.1, 1.0], ndc(30, 40)])
    add("inf_vertex", [ndc(10, 10), ndc(20, 30), [0.1, 0.2, np.inf, 1.5]])
    add("nan_w", [ndc(10, 10), ndc(20, 30), [0.1, 0.2, 0.3, np.nan]])
    add("one_w_negative", [ndc(10, 10), ndc(50, 12), [0.1, 0.3, 0.05, -0.4]])
    add("two_w_negative", [ndc(30, 30, w=0.8), [0.2, -0.1, 0.02, -0.3], [0.1, 0.3, 0.05, -0.4]])
    add("three_w_negative", [[0.2, 0.1, 0.02, -0.5], [0.2, -0.1, 0.02, -0.3], [0.1, 0.3, 0.05, -0.4]])
    add("one_w_zero", [ndc(10, 10), ndc(50, 12), [0.1, 0.3, 0.0, 0.0]])
    add("all_w_zero", [[0.1, 0.2, 0.0, 0.0], [0.3, 0.2, 0.0, 0.0], [0.1, 0.3, 0.0, 0.0]])
    add("beyond_guard_band", [ndc(-40000.0, -30000.0), ndc(50000.0, -20000.0), ndc(100.0, 60000.0)])
    add("near_plane", [ndc(5, 5, z=-1.5), ndc(60, 8, z=0.5), ndc(30, 55, z=0.2)])
    add("behind_near_plane", [ndc(5, 5, z=-1.5), ndc(60, 8, z=-1.2), ndc(30, 55, z=-1.1)])
    add("flat_depth", [ndc(5, 5, z=0.5), ndc(25, 8, z=0.5), ndc(12, 30, z=0.5)])
    v, f = np.concatenate(v), np.concatenate(f)
    f[kinds["index_equals_V"], 2] = len(v)
    return v, f, kinds


def test_edge_faces():
    W, H = 65, 63
    v, f, kinds = _edge_scene(W, H)
    ws, stmts, dec = _run(v, f, W, H, what="edge faces")
    st = stmts[0]
    assert not ws.fused and st.oob
    face = {name: st.faces[k] for name, k in kinds.items()}
    rec = {name: st.records[k] for name, k in kinds.items()}
    # each face is the kind its name says, by the statement
    for name in ("zero_area", "repeated_vertex", "sliver_between_centres", "row_sliver", "off_frame_in_guard_band",
                 "below_frame"):
        assert face[name][2:] == (1, False) and rec[name].empty, name
    assert rec["zero_area"].tri.D == 0 and rec["repeated_vertex"].tri.D == 0
    assert rec["sliver_between_centres"].tri.D > 0 and rec["off_frame_in_guard_band"].tri.D > 0
    for name in ("index_out_of_range", "index_negative", "index_equals_V", "nan_vertex", "inf_vertex", "nan_w"):
        assert face[name][2:] == (0, False), name
    assert face["index_negative"][1].tolist() == [1.0, 2.5, float(v[1, 3])]
    assert np.isnan(face["nan_w"][1][2]) and face["inf_vertex"][1][2] == 1.5
    for name in ("three_w_negative", "all_w_zero"):
        assert face[name][2:] == (0, True), name
    for name in ("one_w_negative", "two_w_negative", "one_w_zero", "beyond_guard_band"):
        assert face[name][3] and face[name][2] >= 1 and not rec[name].empty, (name, face[name])
    for name in ("near_plane", "behind_near_plane"):  # (z alone sends no face to the clipping path: R4 rejects it)
        assert face[name][2:] == (1, False) and not rec[name].empty, name
    assert face["flat_depth"][2:] == (1, False) and rec["flat_depth"].plane() == "flat"
    # and the kernel's own answers where the statement leaves nothing to a checker's tolerance
    assert int(dec.flag[0]) != 0
    assert dec.fdata[0, kinds["index_negative"]]["v"].tolist() == [-1, int(f[kinds["index_negative"], 1]), 1]


# Faces that five planes cut into 7 and 8 vertices (5 and 6 sub-triangles): xy in units of the guard band, z at w = 1
_MANY_PLANES = [([[-1.98, 0.46], [0.22, 1.03], [1.56, -2.34]], [-0.19, -0.8, -0.22]),
                ([[-2.5, -2.26], [2.55, 1.74], [1.65, 2.61]], [0.04, -1.82, 0.7]),
                ([[-1.87, 1.44], [1.47, 0.36], [0.89, -1.22]], [-1.19, 0.42, -0.7]),
                ([[-1.57, -1.33], [1.72, -0.13], [-0.47, 1.91]], [-0.37, -1.22, -0.23])]


def _clip_case(name):
    if name == "clipping":
        W, H = 96, 64
        _, v, _, f = scenes.clipping_scene(W=W, H=H, C=1)
        extra = np.array([[p[k][0] * 32768.0 / W, p[k][1] * 32768.0 / H, z[k], 1.0] for p, z in _MANY_PLANES
                          for k in range(3)], np.float32)
        f = np.concatenate([f, len(v) + np.arange(len(extra), dtype=np.int32).reshape(-1, 3)])
        return _batched(np.concatenate([v, extra]), f) + (W, H)
    if name.startswith("near_w0_"):
        return _batched(*scenes.near_w0_scene(int(name[8:]), C=1)[1::2]) + (64, 48)
    if name == "vertex_cap":
        return _batched(*scenes.near_w0_scene(41533, W=33, H=17, C=1)[1::2]) + (33, 17)
    assert name == "clamped_sub_vertex"
    scene = scenes.fuzz_case(167059)
    return scene[1], scene[3], scene[0].shape[2], scene[0].shape[1]


CLIP_CASES = ["clipping", "near_w0_3", "near_w0_11", "near_w0_12", "vertex_cap", "clamped_sub_vertex"]
_clip_statements = {}


def _clip_stated(name):
    if name not in _clip_statements:
        v, f, W, H = _clip_case(name)
        _clip_statements[name] = (v, f, W, H, _statements(v, f, W, H))
    return _clip_statements[name]


def test_clipped_cases_show_every_sub_triangle_count():
    """(of the statements alone: what test_clipped_faces below runs covers clipped faces of 0 to 6 sub-triangles)"""
    seen = {n for name in CLIP_CASES[:4] for st in _clip_stated(name)[4] for _, _, n, clipped in st.faces if clipped}
    assert seen == {0, 1, 2, 3, 4, 5, 6}, seen


@pytest.mark.parametrize("name", CLIP_CASES)
def test_clipped_faces(name):
    """scenes.py's clipping and near-w = 0 generators: sub-triangle records with their 1 / w and basis, FaceData of
    clipped faces, the R5 vertex cap (near_w0 seed 41533) and sub-vertex clamp (fuzz seed 167059) with their
    counters."""
    v, f, W, H, stmts = _clip_stated(name)
    ws, stmts, dec = _run(v, f, W, H, what=name, stmts=stmts)
    assert not ws.fused
    assert any(r.clipped and r.s > 0 and not r.empty for st in stmts for r in st.records.values())
    if name == "vertex_cap":
        assert sum(st.cap_culled for st in stmts) >= 1 and int(dec.flag[ws.L["kStatCapCulled"]]) >= 1
    if name == "clamped_sub_vertex":
        assert sum(st.clamped for st in stmts) >= 1 and int(dec.flag[ws.L["kStatClamped"]]) >= 1


# ---- slab overflow


def test_slab_overflow_some_tiles():
    """An explicit small bin_capacity: some slabs overflow and some do not.  The counts are the full counts; an
    overflowed slab holds a duplicate-free part of its tile's set."""
    W, H = 200, 136
    _, v, _, f = scenes.random_triangles(F=300, W=W, H=H, C=1, radius_px=8.0, seed=11)
    v = v.copy()
    v[:200 * 3, :2] = v[:200 * 3, :2] * 0.3 - 0.6  # two thirds of the faces crowd the lower left
    ws, stmts, dec = _run(v, f, W, H, bin_capacity=12 * 24, what="slab overflow")
    L = ws.L
    assert L["slab"] == 24 and not ws.fused
    n = np.array([len(stmts[0].tiles(6).get(c, {})) for c in range(12)])
    assert (n > 24).any() and ((n > 0) & (n <= 24)).any(), n
    np.testing.assert_array_equal(dec.counts[0, 0], n)
    assert n.max() > 2 * 24  # (several workgroups' reservations past the slab's end)


# ---- three forwards on one scratch


def test_three_forwards_on_one_scratch():
    """DIRT_FWD_SCRATCH_CLEAN: the count sets alternate, each setup zeroes the set the forward before it used, and the
    sticky flag words accumulate.  The second geometry leaves fewer entries in every tile than the first, so a count
    or an entry left over from the first would show."""
    from dirt_amd import _lib
    W, H, F = 200, 136, 129
    g1 = scenes.random_triangles(F=F, W=W, H=H, C=1, radius_px=30.0, seed=21)
    g2 = scenes.random_triangles(F=F, W=W, H=H, C=1, radius_px=3.0, seed=21)  # (g1's centres)
    g3 = scenes.random_triangles(F=F, W=W, H=H, C=1, radius_px=14.0, seed=23, perspective=True)
    geoms = []
    for k, g in enumerate((g1, g2, g3)):
        v, f = g[1].copy(), g[3].copy()
        if k == 1:
            v[3 * 64:, 0] += 10.0   # half of the faces off the frame, inside the guard band
            v[6:9, 3] = -0.5        # a face clipped away
            f[5] = [0, 1, 3 * F]    # an index out of range: the flag stays set for the third forward
        geoms.append(_batched(v, f))
    ws = _Workspace(1, H, W, 3 * F, F)
    assert not ws.fused
    sts = [_statements(v, f, W, H) for v, f in geoms]
    t1, t2 = sts[0][0].tiles(6), sts[1][0].tiles(6)
    assert len(t1) == 12 and all(len(t2.get(c, {})) < len(t1[c]) for c in t1)
    assert not sts[0][0].oob and sts[1][0].oob and not sts[2][0].oob
    oob = False
    for k, ((v, f), st) in enumerate(zip(geoms, sts)):
        ws.forward(v, f, flags=_lib.FWD_SCRATCH_CLEAN)
        oob = oob or st[0].oob
        _assert_clean(ss.check(ws.decoded(), ss.Expect(st, binned=k + 1, oob=oob)), "forward %d of 3" % (k + 1))


# ---- the fused small-scene forward


@pytest.mark.parametrize("s", [0, 2, 5])
def test_fused_forward(s):
    """F <= kFusedMaxF in few tiles: the raster kernel's own setup publishes the records and FaceData; it leaves the
    counts, the parity words and the bins as it found them."""
    scene = scenes.adversarial_scene(s, W=33, H=17, C=1, F=8)
    v, f = _batched(scene[1], scene[3])
    ws, stmts, dec = _run(v, f, 33, 17, what="fused seed %d" % s)
    assert ws.fused and ws.F <= ws.L["kFusedMaxF"]
    assert any(clipped and n >= 1 for _, _, n, clipped in stmts[0].faces)
    assert not dec.counts.any() and not dec.bins["ri"].any() and not dec.bins["rel"].any()
    assert int(dec.flag[ws.L["kParP"]]) == 0 and int(dec.flag[ws.L["kParQ"]]) == 0


def test_fused_forward_leaves_nonzero_parity_words_alone():
    """DIRT_FWD_SCRATCH_CLEAN on a scratch whose parity words are as two binned forwards leave them (P = 1, Q = 0):
    a fused forward leaves the words and the zero counts as it found them."""
    from dirt_amd import _lib
    scene = scenes.adversarial_scene(2, W=33, H=17, C=1, F=8)
    v, f = _batched(scene[1], scene[3])
    ws = _Workspace(1, 17, 33, v.shape[1], f.shape[1])
    assert ws.fused
    L = ws.L
    words = ws.scratch[L["off_flag"]:L["off_flag"] + 256].view(torch.int32)
    words[L["kParP"]], words[L["kParQ"]] = 1, 0
    ws.forward(v, f, flags=_lib.FWD_SCRATCH_CLEAN)
    dec = ws.decoded()
    assert int(dec.flag[L["kParP"]]) == 1 and int(dec.flag[L["kParQ"]]) == 0 and not dec.counts.any()
    _assert_clean(ss.check(dec, ss.Expect(_statements(v, f, 33, 17), binned=0, parity=(1, 0))), "fused, P = 1")


# ---- the stash forward


def test_stash_forward():
    """dirt_rasterise_fwd_stash: the records and FaceData at the head of the recompute workspace (and the scratch
    behind them) are those of the same statement."""
    from dirt_amd import _lib
    W, H = 96, 64
    v, f = _batched(*scenes.clipping_scene(W=W, H=H, C=1)[1::2])
    B, V, F = 1, v.shape[1], f.shape[1]
    L = _lib.debug_layout(B, H, W, F, 0)
    nbytes = _lib.recompute_workspace_size(B, H, W, 1, V, F)
    wsb = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    bg, cols = torch.zeros((B, H, W, 1), device="cuda"), torch.ones((B, V, 1), device="cuda")
    pixels = torch.empty((B, H, W, 1), device="cuda")
    vt, ft = _gpu(v), _gpu(f)
    _lib.check(_lib.load().dirt_rasterise_fwd_stash(bg.data_ptr(), vt.data_ptr(), cols.data_ptr(), ft.data_ptr(), B, H,
                                                    W, 1, V, F, pixels.data_ptr(), wsb.data_ptr(), nbytes, 0,
                                                    _stream()))
    torch.cuda.synchronize()
    host = wsb.cpu().numpy()
    off_scratch = (L["saved_total"] + 255) // 256 * 256
    dec = ss.decode(L, B, F, host[:L["saved_total"]], host[off_scratch:off_scratch + L["scratch_total"]])
    assert F > L["kFusedMaxF"]
    _assert_clean(ss.check(dec, ss.Expect(_statements(v, f, W, H), binned=1)), "stash forward")
