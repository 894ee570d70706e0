"""Statement of record for the cube-map lookup (dirt_amd.deferred.sample_cubemap, dirt_amd/csrc/cubemap_kernels.h),
and its table of cases.  numpy only, no torch and no code shared with either implementation; the per-axis filtering
rule is texture_cases._axis (the statement of a texture level), the face rule is restated here.  TEST
INFRASTRUCTURE ONLY.

Rule, in the arithmetic `dtype` (float32: the kernels' statement, every line one IEEE operation); (x, y, z) a direction:
  major axis: x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z;  ma = that component
  the negative face exactly when ma < 0; faces +x, -x, +y, -y, +z, -z = 0..5, (sc, tc) by the OpenGL table:
    +x: (-z, -y)   -x: (+z, -y)   +y: (+x, +z)   -y: (+x, -z)   +z: (+x, -y)   -z: (-x, -y)
  m = |ma|;  su = sc / m;  sv = tc / m;  u = su + 1;  u = u * 0.5;  v = sv + 1;  v = v * 0.5
  the face filtered at (u, v) by the clamp rule of texture_cases with Th = Tw = S.
A pixel is sampled where the mask is nonzero (None: everywhere) and its direction is finite and not all zero; the
others give exactly 0, no gradient.

sample_vjp takes the forward's float32 coordinates and weights and does every product and sum in float64:
  grad_cubemap[f,face,i0,j0,c] += g_c * (1 - a) * (1 - b)   and likewise for the other three taps
  gu = S * sum_c g_c * ((t01 - t00) * (1 - b) + (t11 - t10) * b);  gv = S * sum_c g_c * (bot_c - top_c)
  g_sc = 0.5 * gu / m;  g_tc = 0.5 * gv / m;  g_ma = sign(ma) * -(0.5 * gu * su + 0.5 * gv * sv) / m
written to x, y, z through the table's signs, with the sums of the absolute terms beside them.
"""
import functools

import numpy as np

import texture_cases as tc
from texture_cases import F32, PATCH_TEXELS, _rng, _yx, tap_box, tiles  # noqa: F401

FACES = ("+x", "-x", "+y", "-y", "+z", "-z")


def coordinates(directions, valid, dt):
    """-> (face int64, ma, m, su, sv, u, v) in dt; unsampled pixels take the direction (1, 1, 1)"""
    d = np.where(valid[..., None], directions, dt(1))
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    ma = np.where(is_x, x, np.where(is_y, y, z))
    neg = ma < 0
    face = np.where(is_x, 0, np.where(is_y, 2, 4)) + neg
    sc = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x)
    tc_ = np.select([face == 2, face == 3], [z, -z], -y)
    m = np.abs(ma)
    su = sc / m
    sv = tc_ / m
    u = su + dt(1)
    u = u * dt(0.5)
    v = sv + dt(1)
    v = v * dt(0.5)
    assert u.dtype == dt and v.dtype == dt
    return face.astype(np.int64), ma, m, su, sv, u, v


def sample(cubemap, directions, mask=None, dtype=F32, fetch=None):
    """cubemap [6,S,S,C] or [Cf,6,S,S,C] (Cf == B), directions [B,H,W,3], mask [B,H,W] or None -> dict: texels
    [B,H,W,C] (dtype), valid [B,H,W] bool, frame, face, the taps i0, i1, j0, j1, the weights a, b, oma, omb and the
    coordinates ma, m, su, sv, u, v, all [B,H,W].  With `fetch`, cubemap is only its 5-D shape and
    fetch(f, face, i, j) -> [B,H,W,C] reads the texels (a cube map too large for the host)."""
    dt = np.dtype(dtype).type
    directions = np.asarray(directions, dt)
    B, H, W, _ = directions.shape
    if fetch is None:
        t = np.asarray(cubemap, dt)
        t = t[None] if t.ndim == 4 else t
        Cf, six, S, S2, C = t.shape
        fetch = lambda f, face, i, j: t[f, face, i, j]  # noqa: E731
    else:
        Cf, six, S, S2, C = cubemap
    assert Cf in (1, B) and six == 6 and S == S2
    valid = np.isfinite(directions).all(-1) & (directions != 0).any(-1)
    if mask is not None:
        valid = valid & (np.asarray(mask).reshape(B, H, W) != 0)
    with np.errstate(invalid="ignore", over="ignore"):
        face, ma, m, su, sv, u, v = coordinates(directions, valid, dt)
    assert np.all((u >= 0) & (u <= 1) & (v >= 0) & (v <= 1))
    j0, j1, a, pu = tc._axis(u, S, "clamp", dt)
    i0, i1, b, pv = tc._axis(v, S, "clamp", dt)
    assert pu.all() and pv.all()
    f = np.zeros((B, 1, 1), np.int64) if Cf == 1 else np.arange(B)[:, None, None]
    oma, omb = dt(1) - a, dt(1) - b
    A, Bw, OA, OB = a[..., None], b[..., None], oma[..., None], omb[..., None]
    top = np.asarray(fetch(f, face, i0, j0), dt) * OA + np.asarray(fetch(f, face, i0, j1), dt) * A
    bot = np.asarray(fetch(f, face, i1, j0), dt) * OA + np.asarray(fetch(f, face, i1, j1), dt) * A
    out = top * OB + bot * Bw
    assert out.dtype == dt
    return {"texels": np.where(valid[..., None], out, dt(0)), "valid": valid, "frame": np.broadcast_to(f, valid.shape),
            "face": face, "i0": i0, "i1": i1, "j0": j0, "j1": j1, "a": a, "b": b, "oma": oma, "omb": omb,
            "ma": ma, "m": m, "su": su, "sv": sv, "u": u, "v": v}


def _to_xyz(face, g_sc, g_tc, g_ma, sign):
    """(g_sc, g_tc, g_ma) written to x, y, z through the table; sign=False drops the signs (absolute sums)"""
    s = -1.0 if sign else 1.0
    gx = np.select([face <= 1, face == 5], [g_ma, s * g_sc], g_sc)
    gy = np.where((face == 2) | (face == 3), g_ma, s * g_tc)
    gz = np.select([face == 0, face == 1, face == 2, face == 3], [s * g_sc, g_sc, g_tc, s * g_tc], g_ma)
    return np.stack([gx, gy, gz], -1)


def sample_vjp(cubemap, grad, fwd):
    """-> dict: grad_cubemap (float64, cubemap's shape), n, S (same shape), grad_directions [B,H,W,3],
    abs_directions [B,H,W,3]"""
    t = np.asarray(cubemap, np.float64)
    shared = t.ndim == 4
    t = t[None] if shared else t
    size = t.shape[2]
    v = fwd["valid"]
    g = np.where(v[..., None], np.asarray(grad, np.float64), 0.0)
    a, b, oma, omb = (np.asarray(fwd[k], np.float64)[..., None] for k in ("a", "b", "oma", "omb"))
    f, face, i0, i1, j0, j1 = (fwd[k] for k in ("frame", "face", "i0", "i1", "j0", "j1"))
    gt, n, S = np.zeros(t.shape), np.zeros(t.shape, np.int64), np.zeros(t.shape)
    for ii, jj, w in ((i0, j0, oma * omb), (i0, j1, a * omb), (i1, j0, oma * b), (i1, j1, a * b)):
        term = (g * w)[v]
        idx = (f[v], face[v], ii[v], jj[v])
        np.add.at(gt, idx, term)
        np.add.at(S, idx, np.abs(term))
        np.add.at(n, idx, (term != 0).astype(np.int64))
    t00, t01, t10, t11 = t[f, face, i0, j0], t[f, face, i0, j1], t[f, face, i1, j0], t[f, face, i1, j1]
    du = (t01 - t00) * omb + (t11 - t10) * b
    top, bot = t00 * oma + t01 * a, t10 * oma + t11 * a
    gu = size * (g * du).sum(-1)
    gv = size * (g * (bot - top)).sum(-1)
    au = size * (np.abs(g) * (np.abs(t01 - t00) * omb + np.abs(t11 - t10) * b)).sum(-1)
    av = size * (np.abs(g) * ((np.abs(t00) + np.abs(t10)) * oma + (np.abs(t01) + np.abs(t11)) * a)).sum(-1)
    ma, m, su, sv = (np.asarray(fwd[k], np.float64) for k in ("ma", "m", "su", "sv"))
    hu, hv = 0.5 * gu, 0.5 * gv
    g_m = -((hu * su + hv * sv) / m)
    g_ma = np.where(ma < 0, -g_m, g_m)
    gd = _to_xyz(face, hu / m, hv / m, g_ma, True)
    ad = _to_xyz(face, 0.5 * au / m, 0.5 * av / m, (0.5 * au * np.abs(su) + 0.5 * av * np.abs(sv)) / m, False)
    out = {"grad_cubemap": gt, "n": n, "S": S, "grad_directions": np.where(v[..., None], gd, 0.0),
           "abs_directions": np.where(v[..., None], ad, 0.0)}
    if shared:
        out.update({k: out[k][0] for k in ("grad_cubemap", "n", "S")})
    return out


# ---- bounds

def cubemap_bound(vjp):
    """texture_cases.texture_bound: a term g * w1 * w2 is two float32 products, n terms take n - 1 additions in
    whatever order and grouping, the n-th unit absorbs the second order: (n + 2) * 2^-24 * S."""
    return (vjp["n"] + tc.K_TEXTURE) * 2.0 ** -24 * vjp["S"]


def directions_roundings(C):
    """(gu, gv) are tex_grad_uv's with Th = Tw = S: texture_cases.uv_roundings(C) = C + 5 units, the second-order
    unit among them.  The chain adds: hu = 0.5 * gu is exact (a power of two); g_sc = hu / m and g_tc = hv / m are one
    division each, C + 6 in all.  g_ma's two terms hu * su and hv * sv are one product each (su, sv are the
    forward's float32 values, handed over), then one addition, one division; the two negations are exact: 3 more,
    C + 8 in all.  The larger count serves the three components."""
    return tc.uv_roundings(C) + 3


def directions_bound(vjp, C):
    return directions_roundings(C) * 2.0 ** -24 * vjp["abs_directions"]


# ---- direction patterns: functions of (shape, S, rng) -> float64 [B,H,W,3]

def on_face(face, u, v):
    """the direction with ma = +-1 that the table sends to (u, v) of `face` (an int or an array)"""
    s, t = 2.0 * np.asarray(u, np.float64) - 1.0, 2.0 * np.asarray(v, np.float64) - 1.0
    face = np.broadcast_to(face, s.shape)
    one = np.ones_like(s)
    x = np.select([face == 0, face == 1, face == 5], [one, -one, -s], s)
    y = np.select([face == 2, face == 3], [one, -one], -t)
    z = np.select([face == 0, face == 1, face == 2, face == 3, face == 4], [-s, s, t, -t, one], -one)
    return np.stack([x, y, z], -1)


def _d_random(shape, S, rng):
    """Gaussian directions with lengths over e^-5 .. e^5"""
    return rng.standard_normal(shape + (3,)) * np.exp(rng.uniform(-5.0, 5.0, shape))[..., None]


def _lattice_points():
    grid = (-1.0, 0.0, 1.0)
    pts = [(x, y, z) for x in grid for y in grid for z in grid if (x, y, z) != (0, 0, 0)]
    minus = [tuple(-0.0 if c == 0 else c for c in p) for p in pts if 0.0 in p]  # (the same points, zeros as -0.0)
    return np.array(pts + minus), len(pts)


# the faces of the 26 points in that order, worked out by hand from the rule: x = -1 wins every tie (-x); with x = 0,
# y = -1: -y, (0, 0, -1): -z, (0, 0, 1): +z, y = 1: +y; x = 1: +x.  The -0.0 variants keep their point's face.
LATTICE_FACES = [1] * 9 + [3, 3, 3, 5, 4, 2, 2, 2] + [0] * 9


def lattice_faces(shape):
    pts, n = _lattice_points()
    want = np.array(LATTICE_FACES + [LATTICE_FACES[i] for i, p in enumerate(pts[:n]) if 0.0 in p])
    B, H, W = shape
    return want[np.arange(B * H * W) % len(pts)].reshape(shape)


def _d_lattice(shape, S, rng):
    pts, _ = _lattice_points()
    B, H, W = shape
    return pts[np.arange(B * H * W) % len(pts)].reshape(shape + (3,))


def _d_oneface_magnify(shape, S, rng):
    """a smooth warp moving 1/16 texel per pixel on one face per frame (+z, -x, -y), lengths varying: a 16 x 16 tile
    lands in a 2 x 2 (at most 3 x 3) patch of one face's texels"""
    y, x = _yx(shape)
    u = 0.31 + (x + 0.25 * np.sin(y / 5.0)) / (16.0 * S)
    v = 0.47 + (y + 0.25 * np.cos(x / 7.0)) / (16.0 * S)
    face = np.array([4, 1, 3])[np.arange(shape[0]) % 3][:, None, None]
    return on_face(face, u, v) * (1.5 + np.sin(x / 3.0 + y / 4.0))[..., None]


def _d_oneface_scatter(shape, S, rng):
    """uniform over the -z face: one face, but a tile's footprint is the whole face"""
    u, v = rng.uniform(0.0, 1.0, shape), rng.uniform(0.0, 1.0, shape)
    return on_face(5, u, v) * rng.uniform(0.5, 2.0, shape)[..., None]


def _d_corner(shape, S, rng):
    """every 16 x 16 tile centred on the (+x, +y, +z) corner: the angle about the tile's centre picks the largest
    component, so a tile touches the faces +x, +y and +z"""
    y, x = _yx(shape)
    cy, cx = (y % 16) - 7.5, (x % 16) - 7.5
    th, r = np.arctan2(cy, cx), np.hypot(cy, cx) / 8.0
    return 1.0 + 0.1 * r[..., None] * np.stack([np.cos(th), np.cos(th + 2.1), np.cos(th + 4.2)], -1)


def _d_exact(shape, S, rng):
    """ma = +-1 and sc, tc = k / S - 1 on random faces: u = k / (2 S) exactly (S a power of two)"""
    assert S & (S - 1) == 0
    ku, kv = rng.integers(0, 2 * S + 1, shape), rng.integers(0, 2 * S + 1, shape)
    return on_face(rng.integers(0, 6, shape), ku / (2.0 * S), kv / (2.0 * S))


PATTERNS = {"random": _d_random, "lattice": _d_lattice, "oneface-magnify": _d_oneface_magnify,
            "oneface-scatter": _d_oneface_scatter, "corner": _d_corner, "exact": _d_exact}

# ---- the table

FRAMES = {"1x1": (1, 1, 1), "15x17": (1, 15, 17), "16x16": (1, 16, 16), "17x33": (1, 17, 33), "3x5x6": (3, 5, 6)}
SIZES = [1, 2, 5, 8, 64]
CHANNELS = [1, 3, 4, 8]


# (id, frame, S, C, per-frame cubemap, pattern, holes)
# holes: None = every direction usable; "bg" = pixels at -inf, a NaN, the zero vector, and the second tile of the
# first row (where there is one) all background; "mask" = those, and an explicit mask that is set over some of them
def _table():
    rows = []

    def add(frame, S, C, per_frame, pattern, holes=None):
        ident = "%s-s%d-c%d-%s-%s%s" % (frame, S, C, "perframe" if per_frame else "shared", pattern,
                                         "-" + holes if holes else "")
        rows.append((ident, frame, S, C, per_frame, pattern, holes))

    k = 0
    for frame in FRAMES:
        for S in SIZES:
            add(frame, S, CHANNELS[k % 4], (k // 2) % 2 == 1, "random", (None, "bg", "mask")[k % 3])
            k += 1
    for C in CHANNELS:
        for per_frame in (False, True):
            add("17x33", 5, C, per_frame, "random", "bg")
            add("3x5x6", 5, C, per_frame, "random", "mask")
    for S in (1, 2, 5, 8):
        add("15x17", S, 3, False, "lattice")
    add("17x33", 8, 3, False, "lattice", "mask")
    add("3x5x6", 5, 4, True, "lattice", "bg")
    for S in (1, 2, 8, 64):
        add("15x17", S, 3, False, "exact")
    add("3x5x6", 8, 4, True, "exact", "bg")
    add("16x16", 64, 3, False, "oneface-magnify", "bg")
    add("16x16", 64, 8, False, "oneface-scatter")
    add("16x16", 64, 4, False, "corner")
    for frame in ("16x16", "17x33"):
        add(frame, 8, 1, False, "corner", "mask")
    add("3x5x6", 64, 3, True, "oneface-magnify", "mask")
    add("3x5x6", 64, 3, False, "oneface-magnify")
    # the channel counts the rows above leave out (the kernels are compiled for every C in 1..8), and every count on
    # the patch, on one face's wide box, and on a seam
    for C in range(1, 9):
        add("17x33", 64, C, C % 2 == 0, "oneface-magnify", "bg")
        add("17x33", 64, C, False, "corner", "bg" if C % 2 else None)
        add("17x33", 64, C, False, "oneface-scatter")
    for C in (2, 5, 6, 7):
        add("3x5x6", 5, C, True, "random", "mask")
    return rows


TABLE = _table()
CASE_IDS = [r[0] for r in TABLE]
assert len(set(CASE_IDS)) == len(CASE_IDS)
_ROWS = {r[0]: r for r in TABLE}


@functools.lru_cache(maxsize=None)
def case_input(ident):
    """(cubemap float32, directions float32 [B,H,W,3], mask uint8 [B,H,W] or None, grad float32 [B,H,W,C])"""
    _, frame, S, C, per_frame, pattern, holes = _ROWS[ident]
    shape = FRAMES[frame]
    rng = _rng(ident)
    cubemap = rng.standard_normal(((shape[0],) if per_frame else ()) + (6, S, S, C)).astype(F32)
    d = np.ascontiguousarray(PATTERNS[pattern](shape, S, rng), F32)
    mask = None
    if holes:
        d[rng.random(shape) < 0.25] = -np.inf
        if shape[2] >= 32:
            d[:, :16, 16:32] = -np.inf  # a tile with no sampled pixel
        flat = d.reshape(-1, 3)
        if len(flat) >= 8:
            flat[1, 0] = np.nan          # a NaN in one channel only
            flat[len(flat) // 2, 2] = np.inf
            flat[3] = 0.0                # the zero vector, and its negative
            flat[5] = -0.0
        if holes == "mask":
            mask = (rng.random(shape) < 0.7).astype(np.uint8)
            usable = np.isfinite(d).all(-1) & (d != 0).any(-1)
            if len(flat) >= 8:
                mask.reshape(-1)[[1, 3, 5, len(flat) // 2]] = 1  # set over the NaN, the zeros, the +inf
                assert ((mask != 0) & ~usable).sum() >= 4 and (usable & (mask == 0)).any()
    grad = rng.standard_normal(shape + (C,)).astype(F32)
    return cubemap, d, mask, grad


@functools.lru_cache(maxsize=None)
def case_forward(ident):
    """the forward dict of the float32 statement: computed once per process, treat as read-only"""
    cubemap, d, mask, _ = case_input(ident)
    fwd = sample(cubemap, d, mask)
    _, frame, S, C, per_frame, pattern, holes = _ROWS[ident]
    faces = set(fwd["face"][fwd["valid"]].tolist())
    if pattern == "random" and fwd["valid"].size >= 90:
        assert faces == set(range(6)), (ident, faces)
    if pattern == "lattice":
        assert np.array_equal(fwd["face"][fwd["valid"]], lattice_faces(FRAMES[frame])[fwd["valid"]]), ident
        assert holes or faces == set(range(6))
    if pattern == "corner":
        assert faces == {0, 2, 4}, (ident, faces)
    if pattern == "exact":
        assert set(np.unique(fwd["a"])) <= {0.0, 0.5} and set(np.unique(fwd["b"])) <= {0.0, 0.5}
        assert np.array_equal(fwd["m"], np.ones_like(fwd["m"]))
    if holes and fwd["valid"].size >= 8:
        assert not fwd["valid"].reshape(-1)[[1, 3, 5, fwd["valid"].size // 2]].any(), ident
    return fwd


@functools.lru_cache(maxsize=None)
def case(ident):
    """(inputs, forward dict, vjp dict) of the float32 statement: computed once per process, treat as read-only"""
    inputs, fwd = case_input(ident), case_forward(ident)
    return inputs, fwd, sample_vjp(inputs[0], inputs[3], fwd)


# ---- the exact scatter: weights in {0, 1/4, 1/2, 1}, m = 1, small integer texels and cotangents, so that every
# partial sum of both gradients is exact in float32 and the result does not depend on the order of the atomics

@functools.lru_cache(maxsize=None)
def exact_scatter_case(kind, C=3, frames=1):
    """kind 'patch': half-texel steps every 8 pixels on the +z face (16 pixels per texel: the LDS patch); 'direct':
    random half-texel positions on random faces of the S = 64 cube map (direct atomics).  The cube map is shared:
    with frames > 1 its gradient sums over them.  -> (inputs, forward dict, vjp dict)"""
    shape, S = (frames, 31, 33), 64
    rng = _rng("exact-cube", kind, C, frames)
    if kind == "patch":
        y, x = _yx(shape)
        d = on_face(4, (37 + x // 8) / (2.0 * S), (51 + y // 8) / (2.0 * S))
    else:
        d = _d_exact(shape, S, rng)
    d = d.astype(F32)
    d[:, 3, 4] = -np.inf
    cubemap = rng.integers(-2, 3, (6, S, S, C)).astype(F32)
    grad = rng.integers(-3, 4, shape + (C,)).astype(F32)
    fwd = sample(cubemap, d)
    assert set(np.unique(fwd["a"])) <= {0.0, 0.5} and set(np.unique(fwd["b"])) <= {0.0, 0.5}
    disp = dispositions(fwd)
    assert (disp["patch"] > 0 and disp["direct"] == 0) if kind == "patch" else disp["direct"] > 0
    return (cubemap, d, None, grad), fwd, sample_vjp(cubemap, grad, fwd)


# ---- coverage conditions, asserted at import so that the table cannot quietly miss them.  How the backward treats a
# 16 x 16 screen tile follows from the statement alone: the faces of the tile's sampled pixels and the bounding box of
# their taps against the LDS budget (texture_cases.PATCH_TEXELS, which the cube kernel shares).
DISPOSITIONS = ("patch", "direct", "direct_seam", "direct_box", "empty")  # (direct = direct_seam + direct_box)


def dispositions(fwd):
    """-> {disposition: tiles} of one forward dict"""
    n = dict.fromkeys(DISPOSITIONS, 0)
    for sl in tiles(fwd["valid"].shape):
        v = fwd["valid"][sl]
        box = tap_box(v, *(fwd[k][sl] for k in ("i0", "i1", "j0", "j1")))
        if box is None:
            n["empty"] += 1
        elif len(set(fwd["face"][sl][v].tolist())) > 1:
            n["direct"] += 1
            n["direct_seam"] += 1
        elif box[2] * box[3] > PATCH_TEXELS:
            n["direct"] += 1
            n["direct_box"] += 1
        else:
            n["patch"] += 1
    return n


def coverage_counts():
    """-> {C: {disposition: tiles}} over the table"""
    out = {}
    for row in TABLE:
        per_c = out.setdefault(row[3], dict.fromkeys(DISPOSITIONS, 0))
        for k, n in dispositions(case_forward(row[0])).items():
            per_c[k] += n
    return out


def _coverage():
    counts = coverage_counts()
    for C in range(1, 9):
        assert C in counts and all(counts[C][k] > 0 for k in DISPOSITIONS), (C, counts.get(C))


_coverage()
