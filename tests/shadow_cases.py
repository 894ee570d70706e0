"""Statement of record for the shadow-map lookup (dirt_amd.deferred.sample_shadow, dirt_amd/csrc/shadow_kernels.h), and
its table of cases.  numpy only, no torch and no code shared with either implementation.  TEST INFRASTRUCTURE ONLY.

Rule, in the arithmetic `dtype` (float32: the kernels' statement, every line one IEEE operation); depth [Sh,Sw,1] or
[B,Sh,Sw,1] holds the light's clip-space z before the divide (+inf: nothing drawn), M the light's matrix for row
vectors.  For a sampled pixel (mask != 0; mask None: its three position channels finite) with position p, j = 0..3:
  c_j = ((p0 * M[0][j] + p1 * M[1][j]) + p2 * M[2][j]) + M[3][j]                    (cx, cy, cz, cw)
  front = cw > 0;  iw = 1 / cw
  u = (cx * iw) * 0.5 + 0.5;  v = 0.5 - (cy * iw) * 0.5                            (row 0 of the map is its top)
  inside = front && 0 <= u <= 1 && 0 <= v <= 1                                      (a NaN compares false)
A sampled pixel that is not inside is lit: visibility 1, no gradient.  An inside one, for u with T = Sw (v, Sh alike):
  uc = min(max(u, 0), 1);  x = uc * T;  x = x - 0.5;  fx = floor(x);  a = x - fx;  j0 = (int)fx;  j1 = j0 + 1
  j0, j1 clamped into [0, T - 1];  pass_u = 0 <= u <= 1
and with zc = cz - bias, per tap with depth texel d:
  softness == 0:  s = d >= zc ? 1 : 0
  softness  > 0:  t = (d - zc) * (1 / softness) + 1;  s = t < 0 ? 0 : (t > 1 ? 1 : t);  the tap passes where d is
                  finite and 0 <= t <= 1
  visibility = (s00 * (1 - a) + s01 * a) * (1 - b) + (s10 * (1 - a) + s11 * a) * b
Unsampled pixels give exactly 0.

sample_vjp takes what the forward rounded (the taps, a, b, 1 - a, 1 - b, the s values, the pass flags, cx, cy, iw,
1 / softness) and does every product and sum in float64, with g the cotangent at inside pixels and w_tap the product
of the tap's two weights:
  grad_depth[tap] += g * w_tap * (1 / softness)                     at passing taps
  g_cz = -g * (sum over passing taps of w_tap) * (1 / softness)
  g_u = pass_u ? Sw * g * ((s01 - s00) * (1 - b) + (s11 - s10) * b) : 0
  g_v = pass_v ? Sh * g * ((s10 * (1 - a) + s11 * a) - (s00 * (1 - a) + s01 * a)) : 0
  g_cx = g_u * 0.5 * iw;  g_cy = -g_v * 0.5 * iw;  g_cw = -(g_u * 0.5 * cx - g_v * 0.5 * cy) * iw * iw
  grad_positions[r] = sum_j g_c[j] * M[r][j]
  grad_matrix[r][j] = sum over pixels of p_r * g_c[j],  grad_matrix[3][j] = sum over pixels of g_c[j]
and per output element the sum of the absolute terms (every product taken with absolute factors, differences of s
values as |difference| for g_u and as the four s * weight products for g_v) and the number of nonzero terms.
"""
import functools

import numpy as np

F32 = np.float32


def _axis(u, T, dt):
    """the clamp rule of one coordinate -> (i0, i1 int64 in [0, T), a, pass)"""
    with np.errstate(invalid="ignore", over="ignore"):
        uc = np.minimum(np.maximum(u, dt(0)), dt(1))
        ok = (u >= 0) & (u <= 1)
        x = uc * dt(T)
        x = x - dt(0.5)
        fx = np.floor(x)
        a = x - fx
        j0 = np.where(fx >= 0, np.minimum(fx, dt(T)), dt(-1))
    assert a.dtype == dt
    j0 = j0.astype(np.int64)
    return np.clip(j0, 0, T - 1), np.clip(j0 + 1, 0, T - 1), a, ok


def sample(depth, positions, matrix, bias=0.0, softness=0.0, mask=None, dtype=F32):
    """depth [Sh,Sw,1] or [B,Sh,Sw,1], positions [B,H,W,3], matrix [4,4] or [B,4,4], mask [B,H,W] or None -> dict:
    visibility [B,H,W] (dtype), valid, inside [B,H,W] bool and everything sample_vjp needs, all [B,H,W] (s, pass_tap:
    [B,H,W,4] in the order 00, 01, 10, 11)."""
    dt = np.dtype(dtype).type
    pos = np.asarray(positions, dt)
    B, H, W, _ = pos.shape
    d = np.asarray(depth, dt)[..., 0]
    d = d[None] if d.ndim == 2 else d
    Sf, Sh, Sw = d.shape
    assert Sf in (1, B)
    M = np.asarray(matrix, dt)
    M = (M[None] if M.ndim == 2 else M)[:, None, None]  # [1 or B, 1, 1, 4, 4]
    assert M.shape[0] in (1, B)
    valid = np.isfinite(pos).all(-1) if mask is None else (np.asarray(mask).reshape(B, H, W) != 0)
    one, half = dt(1), dt(0.5)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = [((pos[..., 0] * M[..., 0, j] + pos[..., 1] * M[..., 1, j]) + pos[..., 2] * M[..., 2, j]) + M[..., 3, j]
             for j in range(4)]
        cx, cy, cz, cw = c
        iw = one / cw
        u = (cx * iw) * half + half
        v = half - (cy * iw) * half
        inside = valid & (cw > 0) & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    assert u.dtype == dt and v.dtype == dt
    us, vs = np.where(inside, u, dt(0)), np.where(inside, v, dt(0))  # no index from a pixel that is not inside
    j0, j1, a, pu = _axis(us, Sw, dt)
    i0, i1, b, pv = _axis(vs, Sh, dt)
    f = np.zeros((B, 1, 1), np.int64) if Sf == 1 else np.arange(B)[:, None, None]
    f = np.broadcast_to(f, valid.shape)
    taps = np.stack([d[f, i0, j0], d[f, i0, j1], d[f, i1, j0], d[f, i1, j1]], -1)
    inv = dt(0)
    with np.errstate(invalid="ignore", over="ignore"):
        zc = np.where(inside, cz, dt(0)) - dt(bias)
        if softness > 0:
            inv = one / dt(softness)
            t = (taps - zc[..., None]) * inv + one
            s = np.where(t < 0, dt(0), np.where(t > 1, one, t))
            pass_tap = np.isfinite(taps) & (t >= 0) & (t <= 1) & inside[..., None]
        else:
            t = np.full(taps.shape, np.nan, dt)
            s = np.where(taps >= zc[..., None], one, dt(0))
            pass_tap = np.zeros(taps.shape, bool)
        oma, omb = one - a, one - b
        top = s[..., 0] * oma + s[..., 1] * a
        bot = s[..., 2] * oma + s[..., 3] * a
        out = top * omb + bot * b
    assert out.dtype == dt and s.dtype == dt
    vis = np.where(inside, out, np.where(valid, one, dt(0)))
    return {"visibility": vis, "valid": valid, "inside": inside, "frame": f, "i0": i0, "i1": i1, "j0": j0, "j1": j1,
            "a": a, "b": b, "oma": oma, "omb": omb, "s": s, "t": t, "pass_tap": pass_tap, "pass_u": pu & inside,
            "pass_v": pv & inside, "cx": cx, "cy": cy, "cz": cz, "iw": iw, "inv": inv, "Sh": Sh, "Sw": Sw}


def sample_vjp(depth, positions, matrix, grad, fwd):
    """-> dict: grad_depth, n_depth, S_depth (depth's shape); grad_positions, abs_positions [B,H,W,3]; grad_matrix,
    abs_matrix, n_matrix (matrix's shape); all float64 (n: int64)"""
    depth = np.asarray(depth)
    dshape = depth.shape
    d3 = depth[..., 0]
    d3 = d3[None] if d3.ndim == 2 else d3
    M = np.asarray(matrix, np.float64)
    shared_m = M.ndim == 2
    Mb = (M[None] if shared_m else M)[:, None, None]
    ins = fwd["inside"]
    B, H, W = ins.shape
    g = np.where(ins, np.asarray(grad, np.float64).reshape(B, H, W), 0.0)
    a, b, oma, omb, cx, cy, iw = (np.where(ins, np.asarray(fwd[k], np.float64), 0.0)
                                  for k in ("a", "b", "oma", "omb", "cx", "cy", "iw"))
    s = np.where(ins[..., None], np.asarray(fwd["s"], np.float64), 0.0)
    inv = float(fwd["inv"])
    f, i0, i1, j0, j1 = (fwd[k] for k in ("frame", "i0", "i1", "j0", "j1"))
    gd, nd, Sd = np.zeros(d3.shape), np.zeros(d3.shape, np.int64), np.zeros(d3.shape)
    wsum = np.zeros(ins.shape)
    for k, (ii, jj, w) in enumerate(((i0, j0, oma * omb), (i0, j1, a * omb), (i1, j0, oma * b), (i1, j1, a * b))):
        m = fwd["pass_tap"][..., k]
        term = (g * w * inv)[m]
        idx = (f[m], ii[m], jj[m])
        np.add.at(gd, idx, term)
        np.add.at(Sd, idx, np.abs(term))
        np.add.at(nd, idx, (term != 0).astype(np.int64))
        wsum += np.where(m, w, 0.0)
    Sh, Sw = fwd["Sh"], fwd["Sw"]
    s00, s01, s10, s11 = (s[..., k] for k in range(4))
    top, bot = s00 * oma + s01 * a, s10 * oma + s11 * a
    gu = np.where(fwd["pass_u"], Sw * g * ((s01 - s00) * omb + (s11 - s10) * b), 0.0)
    gv = np.where(fwd["pass_v"], Sh * g * (bot - top), 0.0)
    au = np.where(fwd["pass_u"], Sw * np.abs(g) * (np.abs(s01 - s00) * omb + np.abs(s11 - s10) * b), 0.0)
    av = np.where(fwd["pass_v"], Sh * np.abs(g) * ((np.abs(s00) + np.abs(s10)) * oma + (np.abs(s01) + np.abs(s11)) * a),
                  0.0)
    nx, ny = gu * 0.5, gv * -0.5
    gc = np.stack([nx * iw, ny * iw, -g * wsum * inv, -(nx * cx + ny * cy) * iw * iw], -1)
    ac = np.stack([au * 0.5 * np.abs(iw), av * 0.5 * np.abs(iw), np.abs(g) * wsum * inv,
                   (au * 0.5 * np.abs(cx) + av * 0.5 * np.abs(cy)) * iw * iw], -1)
    gp = (gc[..., None, :] * Mb[..., :3, :]).sum(-1)
    ap = (ac[..., None, :] * np.abs(Mb[..., :3, :])).sum(-1)
    p1 = np.concatenate([np.where(ins[..., None], np.asarray(positions, np.float64), 0.0), np.ones((B, H, W, 1))], -1)
    p1 = np.where(ins[..., None], p1, 0.0)
    gm = np.einsum("bhwr,bhwj->brj", p1, gc)
    am = np.einsum("bhwr,bhwj->brj", np.abs(p1), ac)
    nm = np.broadcast_to(ins.sum((1, 2))[:, None, None], gm.shape).astype(np.int64)
    if shared_m:
        gm, am, nm = gm.sum(0), am.sum(0), nm.sum(0)
    return {"grad_depth": gd.reshape(dshape), "n_depth": nd.reshape(dshape), "S_depth": Sd.reshape(dshape),
            "grad_positions": gp, "abs_positions": ap, "grad_matrix": gm, "abs_matrix": am, "n_matrix": nm}


# ---- bounds, in units of 2^-24 times the sum of the absolute terms.  The float64 statement starts from what the
# forward rounded, so only the backward's own float32 operations count (shadow_kernels.h's header has their order).
#
# grad_depth: one term ((g * wa) * wb) * (1 / softness) is three float32 products: k = 3.  n terms are summed by n - 1
# additions whatever their grouping (LDS patch first or not), each rounding a partial sum of at most S(1 + O(2^-24));
# the n-th unit absorbs the second-order terms (texture_cases.texture_bound's argument).
K_DEPTH = 3
# the adjoint of the clip coordinates, the longest path of each:
#   g_cz: the sum inside mt (the products with the 0 / 1 flags are exact), mt * omb, the sum mt * omb + mb * b, the
#         product with g, the product with 1 / softness: 5 (the negation is exact)
#   g_cx: the difference s01 - s00, its product with omb, the sum of the two products, the product with g, the product
#         with Sw: 5; the halving is exact; the product with iw: 6.  g_cy alike through bot - top: 6
#   g_cw: the 5 of g_u, nx * cx, the sum nx * cx + ny * cy, two products with iw: 9
K_CLIP = 9
# grad_positions[r] = ((g_cx * M[r][0] + g_cy * M[r][1]) + g_cz * M[r][2]) + g_cw * M[r][3]: each term one more
# product, then at most three additions, each rounding a partial sum of at most the sum of the absolute terms; one
# unit for the second order: 9 + 1 + 3 + 1
K_POSITIONS = K_CLIP + 5
# grad_matrix[r][j]: one term p_r * g_c[j] is K_CLIP + 1 roundings; the n terms of the pixels inside the frustum are
# summed by n - 1 additions (the zeros of the other pixels add exactly), lanes, waves, tiles and frames in whatever
# fixed grouping; the n-th unit absorbs the second order
K_MATRIX = K_CLIP + 1


def depth_bound(vjp):
    return (vjp["n_depth"] + K_DEPTH) * 2.0 ** -24 * vjp["S_depth"]


def positions_bound(vjp):
    return K_POSITIONS * 2.0 ** -24 * vjp["abs_positions"]


def matrix_bound(vjp):
    return (vjp["n_matrix"] + K_MATRIX) * 2.0 ** -24 * vjp["abs_matrix"]


# ---- the table

FRAMES = {"1x1": (1, 1, 1), "15x17": (1, 15, 17), "63x65": (1, 63, 65), "264x256": (1, 264, 256),
          "2x33x18": (2, 33, 18), "3x5x6": (3, 5, 6)}
MAPS = [(1, 1), (5, 7), (64, 64)]
CLASSES = ("lit", "shadowed", "ramp", "not_inside", "unsampled")


def _rng(*key):
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(str(k))) for k in key])


def _rotation(rng, angle):
    """a rotation by `angle` about a random axis, 3 x 3, for row vectors"""
    k = rng.standard_normal(3)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def light_matrix(kind, rng):
    """An orthographic light over the box |x|, |y| <= 1 (cz = 2 - z', cw = 1), or an OpenGL perspective light at the
    origin looking down -z (near 0.5, far 6, right = top = 0.5: cw = -z'), either after a small random rotation of
    the world and a small shift, so that no entry of the 3 x 4 part that matters is zero by construction."""
    world = np.eye(4)
    world[:3, :3] = _rotation(rng, 0.15)
    world[3, :3] = rng.uniform(-0.05, 0.05, 3)
    if kind == "ortho":
        proj = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, -1.0, 0], [0, 0, 2.0, 1.0]])
    else:
        n, fa, r, t = 0.5, 6.0, 0.5, 0.5
        proj = np.array([[n / r, 0, 0, 0], [0, n / t, 0, 0], [0, 0, -(fa + n) / (fa - n), -1.0],
                         [0, 0, -2 * fa * n / (fa - n), 0]])
    return (world @ proj).astype(F32)


def _yx(shape):
    B, H, W = shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.broadcast_to(y, shape), np.broadcast_to(x, shape)


def _positions_random(shape, kind, Sh, Sw, rng):
    """world positions about 1.2 times as wide as the frustum; under the perspective light one in seven behind it"""
    if kind == "ortho":
        return np.stack([rng.uniform(-1.2, 1.2, shape), rng.uniform(-1.2, 1.2, shape), rng.uniform(-1.0, 1.0, shape)], -1)
    z = rng.uniform(-3.0, 0.5, shape)
    return np.stack([rng.uniform(-1.2, 1.2, shape) * np.abs(z), rng.uniform(-1.2, 1.2, shape) * np.abs(z), z], -1)


def _positions_magnify(shape, kind, Sh, Sw, rng):
    """a smooth sheet moving 1/16 texel per pixel under the orthographic light: a 16 x 16 tile lands in a 2 x 2 (at
    most 3 x 3) patch of texels"""
    y, x = _yx(shape)
    px = -0.4 + 2.0 * (x + 0.25 * np.sin(y / 5.0)) / (16.0 * Sw)
    py = 0.1 + 2.0 * (y + 0.25 * np.cos(x / 7.0)) / (16.0 * Sh)
    return np.stack([px, py, rng.uniform(-1.0, 1.0, shape)], -1)


def _positions_scatter(shape, kind, Sh, Sw, rng):
    """uniform inside the frustum: a tile's footprint is the whole map"""
    return np.stack([rng.uniform(-0.9, 0.9, shape), rng.uniform(-0.9, 0.9, shape), rng.uniform(-1.0, 1.0, shape)], -1)


FAMILIES = {"random": _positions_random, "magnify16": _positions_magnify, "scatter": _positions_scatter}


def _background(shape):
    """the covered pixels of a frame (True): all but a band along the bottom and a block in the top left corner, about
    a quarter of the frame, the band one row higher from frame to frame"""
    y, x = _yx(shape)
    B, H, W = shape
    first = np.ceil(0.8 * H) - np.arange(B)[:, None, None]
    return ~((y >= first) | ((x < 0.25 * W) & (y < 0.3 * H)))


# (id, frame, map size, per-frame map, per-frame matrix, light, soft, biased, family, holes, seed)
# holes: None = every pixel finite; "bg" = -inf background (+ one NaN in a single channel); "mask" = an explicit mask
# that disagrees with finiteness where the position is finite (and the -inf background besides)

# the seeds of the random cases whose default left one of their claimed classes under 5 % of the pixels (with a
# single texel, or two small per-frame maps, the split hangs on a handful of random depths)
_SEEDS = {"63x65-m1x1-ss-ortho-hard-nobias-random-bg": 1, "2x33x18-m1x1-Ps-persp-soft-nobias-random-bg": 5,
          "2x33x18-m5x7-PP-persp-soft-bias-random-bg": 3}


def _table():
    rows = []

    def add(frame, smap, map_pf, mat_pf, light, soft, biased, family="random", holes=None, seed=0):
        ident = "%s-m%dx%d-%s%s-%s-%s-%s-%s%s" % (
            frame, smap[0], smap[1], "P" if map_pf else "s", "P" if mat_pf else "s", light,
            "soft" if soft else "hard", "bias" if biased else "nobias", family, "-" + holes if holes else "")
        rows.append((ident, frame, smap, map_pf, mat_pf, light, soft, biased, family, holes, _SEEDS.get(ident, seed)))

    # every frame x every map size, the light, the ramp, the bias, the holes and the forms cycling
    k = 0
    for frame in ("1x1", "15x17", "63x65", "2x33x18", "3x5x6"):
        batch = FRAMES[frame][0] > 1
        for smap in MAPS:
            add(frame, smap, batch and k % 2 == 1, batch and (k // 2) % 2 == 1, ("ortho", "persp")[k % 2],
                (k // 2) % 2 == 0, k % 3 != 0, "random", ("bg", "mask", None)[k % 3])
            k += 1
    # more than 256 tiles in one frame: the second kernel's strided loop
    add("264x256", (64, 64), False, False, "persp", True, True, "random", "bg")
    # shared and per-frame map and matrix, B = 2 and B = 3, both lights, with and without the ramp
    for frame in ("2x33x18", "3x5x6"):
        for map_pf in (False, True):
            for mat_pf in (False, True):
                add(frame, (5, 7), map_pf, mat_pf, "persp" if map_pf == mat_pf else "ortho", True, True, "random", "bg",
                    seed=1)
                add(frame, (64, 64), map_pf, mat_pf, "ortho" if map_pf == mat_pf else "persp", False, False, "random",
                    "mask", seed=1)
    # a tile's taps fit the LDS patch (magnified), or do not (scattered)
    for frame in ("63x65", "2x33x18"):
        add(frame, (64, 64), False, False, "ortho", True, True, "magnify16", "bg")
        add(frame, (64, 64), False, False, "ortho", True, False, "scatter")
    add("63x65", (64, 64), False, False, "ortho", False, True, "magnify16", "mask")
    return rows


TABLE = _table()
CASE_IDS = [r[0] for r in TABLE]
assert len(set(CASE_IDS)) == len(CASE_IDS), CASE_IDS
_ROWS = {r[0]: r for r in TABLE}


def _smooth_field(Sf, Sh, Sw, rng):
    """values in [0, 1] that vary slowly over a large map (neighbouring taps nearly agree) plus a little noise"""
    i, j = np.meshgrid(np.arange(Sh), np.arange(Sw), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, (Sf, 2, 1, 1))
    field = 0.5 + 0.45 * np.sin(np.pi * i / Sh + ph[:, 0]) * np.cos(np.pi * j / Sw + ph[:, 1])
    return np.clip(field + rng.uniform(-0.04, 0.04, (Sf, Sh, Sw)), 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def case_input(ident):
    """(depth float32, positions float32 [B,H,W,3], matrix float32, bias, softness, mask uint8 [B,H,W] or None,
    grad float32 [B,H,W])"""
    _, frame, (Sh, Sw), map_pf, mat_pf, light, soft, biased, family, holes, seed = _ROWS[ident]
    shape = FRAMES[frame]
    B = shape[0]
    rng = _rng(ident, seed)
    matrix = np.stack([light_matrix(light, rng) for _ in range(B)]) if mat_pf else light_matrix(light, rng)
    pos = np.ascontiguousarray(FAMILIES[family](shape, light, Sh, Sw, rng), F32)
    # the map: between the extremes of the clip z of the pixels inside the frustum (float64, for the generator only)
    probe = sample(np.zeros((Sh, Sw, 1)), pos, matrix, dtype=np.float64)
    inside_z = probe["cz"][probe["inside"]]
    lo, hi = (float(inside_z.min()), float(inside_z.max())) if inside_z.size > 1 else (0.0, 1.0)
    span = max(hi - lo, 0.25)
    Sf = B if map_pf else 1
    depth = (lo + span * _smooth_field(Sf, Sh, Sw, rng)).astype(F32)
    if Sh * Sw > 1:  # nothing drawn there (+inf), and the other infinity: one texel in twenty each, at least one
        special = rng.permutation(Sf * Sh * Sw)[: 2 * max(1, Sf * Sh * Sw // 20)]
        depth.reshape(-1)[special[::2]] = np.inf
        depth.reshape(-1)[special[1::2]] = -np.inf
    depth = depth[..., None] if map_pf else depth[0][..., None]
    softness = 0.12 * span if soft else 0.0
    bias = 0.04 * span if biased else 0.0
    mask = None
    if holes:
        covered = _background(shape)
        pos[~covered] = -np.inf
        flat = pos.reshape(-1, 3)
        if len(flat) >= 4:  # a NaN in one channel only
            flat[1, 0] = np.nan
        if holes == "mask":
            finite = np.isfinite(pos).all(-1)
            mask = (finite & (rng.random(shape) < 0.85)).astype(np.uint8)
            assert finite.sum() < 16 or (finite & (mask == 0)).any()
    grad = rng.standard_normal(shape).astype(F32)
    return depth, pos, matrix, float(F32(bias)), float(F32(softness)), mask, grad


@functools.lru_cache(maxsize=None)
def case_forward(ident):
    """the forward dict of the float32 statement: computed once per process, treat as read-only"""
    depth, pos, matrix, bias, softness, mask, _ = case_input(ident)
    return sample(depth, pos, matrix, bias, softness, mask)


@functools.lru_cache(maxsize=None)
def case(ident):
    """(inputs, forward dict, vjp dict) of the float32 statement: computed once per process, treat as read-only"""
    inputs, fwd = case_input(ident), case_forward(ident)
    return inputs, fwd, sample_vjp(inputs[0], inputs[1], inputs[2], inputs[6], fwd)


def classes(fwd):
    """-> {class: share of the pixels} of one forward dict.  lit / shadowed: inside with visibility exactly 1 / 0;
    ramp: inside with at least one tap strictly between the ramp's ends."""
    ins, vis = fwd["inside"], fwd["visibility"]
    with np.errstate(invalid="ignore"):
        ramp = ins & ((fwd["t"] > 0) & (fwd["t"] < 1)).any(-1)
    n = float(ins.size)
    return {"lit": (ins & (vis == 1)).sum() / n, "shadowed": (ins & (vis == 0)).sum() / n, "ramp": ramp.sum() / n,
            "not_inside": (fwd["valid"] & ~ins).sum() / n, "unsampled": (~fwd["valid"]).sum() / n}


def claimed_classes(ident):
    """the classes a random case claims to cover with at least 5 % of its pixels each (frames of at least 15 x 17)"""
    _, frame, _, _, _, _, soft, _, family, holes, _ = _ROWS[ident]
    if family != "random" or FRAMES[frame][1] * FRAMES[frame][2] < 255:
        return ()
    return tuple(c for c in CLASSES if (c != "ramp" or soft) and (c != "unsampled" or holes))


RANDOM_CASE_IDS = [r[0] for r in TABLE if claimed_classes(r[0])]


# ---- the exact scatter: weights in {0, 1/4, 1/2, 1}, 1 / softness = 4, depths and positions in eighths and small
# integer cotangents, so that every partial sum of the depth gradient is exact in float32 and the result does not
# depend on the order of the atomics

@functools.lru_cache(maxsize=None)
def exact_scatter_case(kind, frames=1):
    """kind 'magnify16': half-texel steps every 8 pixels (16 pixels per texel: the LDS patch); 'scatter': random
    half-texel positions over the 64 x 64 map (direct atomics).  -> (inputs, forward dict, vjp dict)"""
    shape, T = (frames, 63, 65), 64
    rng = _rng("exact", kind, frames)
    if kind == "magnify16":
        y, x = _yx(shape)
        ku, kv = 37 + (x // 8).astype(np.int64), 51 + (y // 8).astype(np.int64)
    else:
        ku, kv = rng.integers(1, 2 * T, shape), rng.integers(1, 2 * T, shape)
    # the identity matrix: u = px * 0.5 + 0.5 = k / (2 T) and v = 0.5 - py * 0.5 exactly; x = k / 2 - 0.5: a in {0, 0.5}
    pos = np.stack([ku / float(T) - 1.0, 1.0 - kv / float(T), rng.integers(0, 9, shape) / 8.0], -1).astype(F32)
    pos[:, 3, 4] = -np.inf
    depth = (rng.integers(0, 9, (T, T, 1)) / 8.0).astype(F32)
    depth[5, 6] = np.inf
    grad = rng.integers(-3, 4, shape).astype(F32)
    matrix = np.eye(4, dtype=F32)
    fwd = sample(depth, pos, matrix, 0.0, 0.25, None)
    assert set(np.unique(fwd["a"])) <= {0.0, 0.5} and set(np.unique(fwd["b"])) <= {0.0, 0.5}
    assert fwd["pass_tap"].mean() > 0.1
    return (depth, pos, matrix, 0.0, 0.25, None, grad), fwd, sample_vjp(depth, pos, matrix, grad, fwd)


# ---- how the backward treats a 16 x 16 screen tile follows from the statement alone: the bounding box of the taps
# of the tile's lanes with a passing tap, against the LDS budget (DIRT_TEXTURE_PATCH of
# dirt_amd/csrc/texture_kernels.h, restated here: a changed kernel budget is a table change)
TILE = 16
PATCH_TEXELS = 576
DISPOSITIONS = ("patch", "direct", "empty")


def dispositions(fwd):
    """-> {disposition: tiles} of one forward dict"""
    n = dict.fromkeys(DISPOSITIONS, 0)
    B, H, W = fwd["valid"].shape
    adds = fwd["pass_tap"].any(-1)
    for b in range(B):
        for ty in range(0, H, TILE):
            for tx in range(0, W, TILE):
                sl = (b, slice(ty, ty + TILE), slice(tx, tx + TILE))
                m = adds[sl]
                if not m.any():
                    n["empty"] += 1
                    continue
                r = np.concatenate([fwd["i0"][sl][m], fwd["i1"][sl][m]])
                c = np.concatenate([fwd["j0"][sl][m], fwd["j1"][sl][m]])
                fits = (r.max() - r.min() + 1) * (c.max() - c.min() + 1) <= PATCH_TEXELS
                n["patch" if fits else "direct"] += 1
    return n
