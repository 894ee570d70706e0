"""Statement of record for the seamless mip-mapped cube-map lookup (dirt_amd.deferred.build_cubemap_mipmaps /
sample_cubemap_mip, dirt_amd/csrc/cubemap_mip_kernels.h), and its table of cases.  numpy only, no torch and no code
shared with either implementation.  The face rule is cubemap_cases.coordinates, the chain of a face
texture_mip_cases.build_chain, the lod's tail texture_mip_cases' (restated: it is fused with the uv differences there).
TEST INFRASTRUCTURE ONLY.

Layout.  A chain is the list of its levels, each [6,T,T,C] (shared) or [Cf,6,T,T,C]; packed [.., 6, N, C], face-major.

Rule, in the arithmetic `dtype` (float32: the kernels' statement, every line one IEEE operation); (x, y, z) a sampled
direction, face, ma, m, su, sv, u, v by cubemap_cases.coordinates:
  lod, explicit: the pixel's lod, a NaN counting as 0.
  lod, automatic: P = (x / m, y / m, z / m); the x-difference e = P[y,x+1] - P[y,x] if x+1 < W and that neighbour is
    sampled (branch 0), else P[y,x] - P[y,x-1] if x >= 1 and that neighbour is sampled (branch 1), else 0 (branch 2);
    the y-difference alike;  h = 0.5 * S;  e = e * h;  q = ex * ex;  t = ey * ey;  q = q + t;  t = ez * ez;  q = q + t
    rho2 = fmax(qx, qy) = m * 2^e (frexp);  lod = 0.5 * (e + (m - 1));  0 unless rho2 >= 1;  L-1 when rho2 is inf
  lod = lod + lod_bias, clamped to [0, L-1];  k0 = floor(lod), f = lod - k0, k1 = min(k0+1, L-1)
  taps at level k, T = S_k:  x = u * T;  x = x - 0.5;  fx = floor(x);  a = x - fx;  j0 = (int)fx;  j1 = j0 + 1; i0, i1,
    b from v alike.  seamless=False: the indices clamped to [0, T-1].  seamless=True: `resolve` below, in integers.
  a corner tap (both indices out of range) has the value ((t_p + t_q) + t_r) * third, third = float32(1/3), over the
    other three taps in the order 00, 01, 10, 11
  top = t00 * (1-a) + t01 * a;  bot = t10 * (1-a) + t11 * a;  s_k = top * (1-b) + bot * b
  out = s_k0 * (1-f) + s_k1 * f, and out = s_k0 when f == 0.  Unsampled pixels: exactly 0.

sample_vjp takes the forward's float32 coordinates, weights (a, b, 1-a, 1-b per level, f, 1-f, third) and does every
product and sum in float64:
  grad_packed[resolved tap, c] += g_c * w1 * w2 * wl     wl = 1-f at k0 (1 when f == 0), f at k1 (absent when f == 0);
    a corner tap's term times third, to each of its three source texels
  (gu, gv) per level in the difference form on the tap values (a corner tap's value its float64 mean), blended by
    1-f and f, then cubemap_cases' direction lines
  grad_lod = pass ? sum_c g_c * (s_k1,c - s_k0,c) : 0;  pass: the given lod is not NaN and 0 <= lod + bias <= L-1 (in
    float32, as the rule forms it);  s_k1 is read at f == 0 too (the derivative to the right);  k1 == k0 gives 0
with the sums of the absolute terms beside each.
"""
import functools

import numpy as np

import cubemap_cases as cc
import texture_cases as tc
import texture_mip_cases as tmc

F32 = np.float32
FRAMES = cc.FRAMES
SIZES = cc.SIZES
U = 2.0 ** -24  # the unit roundoff of float32


# ---- chain

def build_chain(cubemap, levels=None, dtype=F32):
    """cubemap [6,S,S,C] or [Cf,6,S,S,C] -> the list of levels, each of cubemap's rank: the faces are the frames of
    texture_mip_cases.build_chain"""
    return tmc.build_chain(cubemap, levels, dtype)


def pack(chain):
    return tmc.pack(chain)


# ---- taps

def _axis(u, T, dt):
    """-> (j0 int64 in [-1, T-1], a): unreduced"""
    x = u * dt(T)
    x = x - dt(0.5)
    fx = np.floor(x)
    a = x - fx
    assert a.dtype == dt
    return np.where(fx >= 0, np.minimum(fx, dt(T - 1)), dt(-1)).astype(np.int64), a


def resolve(face, i, j, T):
    """Tap (i, j) of `face` at a level of T x T faces, i and j in [-1, T] -> (face', i', j', kind): kind 0 in range (the
    tap itself), 1 folded over an edge onto the neighbouring face, 2 a cube corner (no texel; the indices are
    placeholders).  sc = 2j + 1 - T, tc = 2i + 1 - T and the inverse table with major T give the tap's point; the
    coordinate of magnitude T + 1 becomes +-T and the major axis, the old major +-(T - 1); the forward table gives
    (face', sc', tc'), j' = (sc' + T - 1) / 2, i' = (tc' + T - 1) / 2."""
    face, i, j = np.broadcast_arrays(np.asarray(face, np.int64), np.asarray(i, np.int64), np.asarray(j, np.int64))
    oi, oj = (i < 0) | (i >= T), (j < 0) | (j >= T)
    sc, tc_ = 2 * j + 1 - T, 2 * i + 1 - T
    big = np.full(face.shape, T, np.int64)
    p = np.stack([np.select([face == 0, face == 1, face == 5], [big, -big, -sc], sc),
                  np.select([face == 2, face == 3], [big, -big], -tc_),
                  np.select([face == 0, face == 1, face == 2, face == 3, face == 4], [-sc, sc, tc_, -tc_, big], -big)],
                 -1)
    old = face // 2
    past = np.abs(p) == T + 1                      # the coordinate over the edge
    is_old = np.arange(3) == old[..., None]
    sign = np.where(p < 0, -1, 1)
    p2 = np.where(past, sign * T, np.where(is_old, sign * (T - 1), p))
    new = np.argmax(past, -1)                      # (meaningful for kind 1 only)
    ma = np.take_along_axis(p2, new[..., None], -1)[..., 0]
    face2 = 2 * new + (ma < 0)
    x, y, z = p2[..., 0], p2[..., 1], p2[..., 2]
    sc2 = np.select([face2 == 0, face2 == 1, face2 == 5], [-z, z, -x], x)
    tc2 = np.select([face2 == 2, face2 == 3], [z, -z], -y)
    kind = oi.astype(np.int64) + oj
    one = kind == 1
    assert np.all((past.sum(-1) == 1)[one])
    assert np.all((((sc2 + T - 1) % 2) == 0)[one]) and np.all((((tc2 + T - 1) % 2) == 0)[one])
    rf = np.where(one, face2, face)
    ri = np.where(one, (tc2 + T - 1) // 2, np.clip(i, 0, T - 1))
    rj = np.where(one, (sc2 + T - 1) // 2, np.clip(j, 0, T - 1))
    assert np.all((ri >= 0) & (ri < T) & (rj >= 0) & (rj < T) & (rf >= 0) & (rf < 6))
    assert np.all((rf != face)[one])
    return rf, ri, rj, kind


_ORDER = ((0, 0), (0, 1), (1, 0), (1, 1))


def level_sample(level, frame, face, u, v, sel, seamless, dt):
    """One level ([Cf,6,T,T,C], values in any dtype) at the pixels in `sel` -> dict: texels [B,H,W,C] in dt (0 outside
    sel), the four taps' rf, ri, rj, kind (lists of [B,H,W]), the rows and columns r0, r1, c0, c1 on the pixel's own
    face (unreduced, or clamped when not seamless), a, b, oma, omb"""
    T = level.shape[-2]
    c0, a = _axis(u, T, dt)
    r0, b = _axis(v, T, dt)
    r1, c1 = r0 + 1, c0 + 1
    if not seamless:
        r0, c0, r1, c1 = np.maximum(r0, 0), np.maximum(c0, 0), np.minimum(r1, T - 1), np.minimum(c1, T - 1)
    taps = [resolve(face, (r0, r1)[di], (c0, c1)[dj], T) for di, dj in _ORDER]
    assert np.all(sum((t[3] == 2).astype(int) for t in taps) <= 1)  # at most one corner tap
    vals = tap_values(level, frame, taps, dt)
    oma, omb = dt(1) - a, dt(1) - b
    A, Bw, OA, OB = a[..., None], b[..., None], oma[..., None], omb[..., None]
    top = vals[0] * OA + vals[1] * A
    bot = vals[2] * OA + vals[3] * A
    out = top * OB + bot * Bw
    assert out.dtype == dt
    return {"texels": np.where(sel[..., None], out, dt(0)), "sel": sel, "T": T,
            "rf": [t[0] for t in taps], "ri": [t[1] for t in taps], "rj": [t[2] for t in taps],
            "kind": [t[3] for t in taps], "r0": r0, "r1": r1, "c0": c0, "c1": c1, "a": a, "b": b, "oma": oma,
            "omb": omb}


def tap_values(level, frame, taps, dt, absolute=False, third=None):
    """the four tap values [B,H,W,C] in dt, a corner tap's the mean of the other three; third = 1 / 3 formed in dt (the
    rule in that arithmetic) unless one is handed over"""
    third = dt(1) / dt(3) if third is None else dt(third)
    lv = np.asarray(level, dt)
    lv = np.abs(lv) if absolute else lv
    raw = [lv[frame, rf, ri, rj] for rf, ri, rj, _ in taps]
    vals = []
    for n in range(4):
        p, q, r = [k for k in range(4) if k != n]
        mean = raw[p] + raw[q]
        mean = mean + raw[r]
        mean = mean * third
        vals.append(np.where((taps[n][3] == 2)[..., None], mean, raw[n]))
    return vals


# ---- level of detail

def _point(directions, valid, dt):
    d = np.where(valid[..., None], directions, dt(1))
    m = np.abs(d).max(-1, keepdims=True)
    P = d / m
    assert P.dtype == dt
    return P


def lod_of(directions, valid, face, S, L, lod=None, lod_bias=0.0, dtype=F32):
    """-> dict: lod [B,H,W] (the final one, 0 at unsampled pixels), raw (before the clamp, NaN -> 0 and bias applied),
    branch_x, branch_y (2 everywhere with an explicit lod), other_face (the neighbour an automatic difference used
    lies on another face), nan (an explicit NaN), passes (the lod's gradient passes)"""
    dt = np.dtype(dtype).type
    bx = by = np.full(valid.shape, 2, np.int8)
    other = np.zeros(valid.shape, bool)
    nan = np.zeros(valid.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if lod is None:
            P = _point(np.asarray(directions, dt), valid, dt)
            h = dt(0.5) * dt(S)
            q = []
            for axis in (2, 1):
                e, br = tmc._difference(P, valid, axis)
                e = e * h
                qd = e[..., 0] * e[..., 0]
                t = e[..., 1] * e[..., 1]
                qd = qd + t
                t = e[..., 2] * e[..., 2]
                qd = qd + t
                q.append(qd)
                nxt, prv = np.roll(face, -1, axis), np.roll(face, 1, axis)
                other |= ((br == 0) & (nxt != face)) | ((br == 1) & (prv != face))
                if axis == 2:
                    bx = br
                else:
                    by = br
            rho2 = np.fmax(q[0], q[1])
            assert rho2.dtype == dt
            m, e = np.frexp(np.where(np.isfinite(rho2), rho2, dt(1)))
            m = m * dt(2)
            e = (e - 1).astype(dt)
            lod = dt(0.5) * (e + (m - dt(1)))
            lod = np.where(rho2 >= 1, lod, dt(0))
            lod = np.where(np.isinf(rho2), dt(L - 1), lod)
            passes = np.zeros(valid.shape, bool)
        else:
            lod = np.asarray(lod, dt).reshape(valid.shape)
            nan = np.isnan(lod)
            lod = np.where(nan, dt(0), lod)
            passes = ~nan
        raw = lod + dt(lod_bias)
        passes = passes & (raw >= 0) & (raw <= L - 1) & valid
        lod = np.minimum(np.maximum(raw, dt(0)), dt(L - 1))
    assert lod.dtype == dt
    return {"lod": np.where(valid, lod, dt(0)), "raw": raw, "branch_x": bx, "branch_y": by, "other_face": other & valid,
            "nan": nan & valid, "passes": passes}


# ---- lookup

def sample(chain, directions, mask=None, lod=None, lod_bias=0.0, seamless=True, dtype=F32):
    """chain: the list of levels ([6,T,T,C] shared, or [Cf,6,T,T,C] with Cf == B); directions [B,H,W,3]; mask, lod
    [B,H,W] or None -> dict: texels [B,H,W,C], valid, lod, k0, k1, f, omf, blend, above (k1 != k0), frame, face and
    cubemap_cases.coordinates' ma, m, su, sv, u, v, the lod dict's entries, levels {k: level_sample's dict at level k
    for the pixels whose k0 or k1 it is (k1 wherever it differs from k0, read or not)}"""
    dt = np.dtype(dtype).type
    directions = np.asarray(directions, dt)
    B, H, W, _ = directions.shape
    chain = [np.asarray(c)[None] if np.asarray(c).ndim == 4 else np.asarray(c) for c in chain]
    Cf, six, S, _, C = chain[0].shape
    L = len(chain)
    assert Cf in (1, B) and six == 6
    valid = np.isfinite(directions).all(-1) & (directions != 0).any(-1)
    if mask is not None:
        valid = valid & (np.asarray(mask).reshape(B, H, W) != 0)
    with np.errstate(invalid="ignore", over="ignore"):
        face, ma, m, su, sv, u, v = cc.coordinates(directions, valid, dt)
    frame = np.broadcast_to(np.zeros((B, 1, 1), np.int64) if Cf == 1 else np.arange(B)[:, None, None], valid.shape)
    out = lod_of(directions, valid, face, S, L, lod, lod_bias, dtype)
    k0f = np.floor(out["lod"])
    f = out["lod"] - k0f
    omf = dt(1) - f
    k0 = k0f.astype(np.int64)
    k1 = np.minimum(k0 + 1, L - 1)
    blend = valid & (f != 0)
    above = valid & (k1 != k0)
    s0, s1, levels = np.zeros((B, H, W, C), dt), np.zeros((B, H, W, C), dt), {}
    for k in range(L):
        at0, at1 = valid & (k0 == k), above & (k1 == k)
        if not (at0 | at1).any():
            continue
        levels[k] = level_sample(np.asarray(chain[k], dt), frame, face, u, v, at0 | at1, seamless, dt)
        s0 = np.where(at0[..., None], levels[k]["texels"], s0)
        s1 = np.where(at1[..., None], levels[k]["texels"], s1)
    with np.errstate(invalid="ignore", over="ignore"):
        mixed = s0 * omf[..., None] + s1 * f[..., None]
    texels = np.where(valid[..., None], np.where(blend[..., None], mixed, s0), dt(0))
    assert texels.dtype == dt
    out.update(texels=texels, valid=valid, k0=k0, k1=k1, f=f, omf=omf, blend=blend, above=above, frame=frame, face=face,
               ma=ma, m=m, su=su, sv=sv, u=u, v=v, levels=levels, seamless=seamless, third=dt(1) / dt(3))
    return out


def _level_vjp(level, g, wl, lv, frame, third):
    """One level's part, float64: g [B,H,W,C] the cotangent, wl [B,H,W] the level weight (0: the pixel does not add
    here) -> (grad_level, n, S of level's shape; the tap values and their absolute counterparts)"""
    t = np.asarray(level, np.float64)
    gt, n, S = np.zeros(t.shape), np.zeros(t.shape, np.int64), np.zeros(t.shape)
    a, b, oma, omb = (np.asarray(lv[k], np.float64)[..., None] for k in ("a", "b", "oma", "omb"))
    adds = lv["sel"] & (wl != 0)
    third = np.float64(third)  # (the forward's constant, handed over like its weights)
    for num, (di, dj) in enumerate(_ORDER):
        w = (a if dj else oma) * (b if di else omb)
        term = g * w * wl[..., None]
        kind = lv["kind"][num]
        direct = adds & (kind != 2)
        idx = (frame[direct], lv["rf"][num][direct], lv["ri"][num][direct], lv["rj"][num][direct])
        np.add.at(gt, idx, term[direct])
        np.add.at(S, idx, np.abs(term[direct]))
        np.add.at(n, idx, (term[direct] != 0).astype(np.int64))
        corner = adds & (kind == 2)
        if corner.any():
            for other in range(4):
                if other == num:
                    continue
                idx = (frame[corner], lv["rf"][other][corner], lv["ri"][other][corner], lv["rj"][other][corner])
                np.add.at(gt, idx, term[corner] * third)
                np.add.at(S, idx, np.abs(term[corner]) * third)
                np.add.at(n, idx, (term[corner] != 0).astype(np.int64))
    taps = list(zip(lv["rf"], lv["ri"], lv["rj"], lv["kind"]))
    return gt, n, S, tap_values(t, frame, taps, np.float64, False, third), \
        tap_values(t, frame, taps, np.float64, True, third)


def sample_vjp(chain, grad, fwd, lod_given=True):
    """-> dict: grad_packed, n, S ([6,N,C] or [Cf,6,N,C]: float64 / int64 / float64), grad_directions, abs_directions
    [B,H,W,3], grad_lod, abs_lod [B,H,W] (zero without an explicit lod)"""
    shared = np.asarray(chain[0]).ndim == 4
    chain = [np.asarray(c)[None] if shared else np.asarray(c) for c in chain]
    L = len(chain)
    v = fwd["valid"]
    g = np.where(v[..., None], np.asarray(grad, np.float64), 0.0)
    f, omf = fwd["f"].astype(np.float64), fwd["omf"].astype(np.float64)
    frame = fwd["frame"]
    gp, n, S = [], [], []
    shape = v.shape
    gu, gv, au, av = (np.zeros(shape) for _ in range(4))
    s0, s1, a0, a1 = (np.zeros(shape + g.shape[-1:]) for _ in range(4))
    for k in range(L):
        t = np.asarray(chain[k], np.float64)
        if k not in fwd["levels"]:
            gp.append(np.zeros(t.shape)), n.append(np.zeros(t.shape, np.int64)), S.append(np.zeros(t.shape))
            continue
        lv = fwd["levels"][k]
        T = lv["T"]
        at0, at1 = v & (fwd["k0"] == k), fwd["above"] & (fwd["k1"] == k)
        wl = np.where(at0, np.where(fwd["blend"], omf, 1.0), 0.0) + np.where(at1 & fwd["blend"], f, 0.0)
        gk, nk, Sk, tv, ta = _level_vjp(t, g, wl, lv, frame, fwd["third"])
        gp.append(gk), n.append(nk), S.append(Sk)
        a, b, oma, omb = (np.asarray(lv[key], np.float64)[..., None] for key in ("a", "b", "oma", "omb"))
        du = (tv[1] - tv[0]) * omb + (tv[3] - tv[2]) * b
        top, bot = tv[0] * oma + tv[1] * a, tv[2] * oma + tv[3] * a
        gu += wl * T * (g * du).sum(-1)
        gv += wl * T * (g * (bot - top)).sum(-1)
        # the absolute terms: of the texel differences where every tap is a texel (texture_cases' form); of the taps
        # themselves where one is a corner's mean, whose own roundings are relative to its three terms
        has_corner = np.any([kd == 2 for kd in lv["kind"]], 0)[..., None]
        adu = np.where(has_corner, (ta[1] + ta[0]) * omb + (ta[3] + ta[2]) * b,
                       np.abs(tv[1] - tv[0]) * omb + np.abs(tv[3] - tv[2]) * b)
        au += wl * T * (np.abs(g) * adu).sum(-1)
        av += wl * T * (np.abs(g) * ((ta[0] + ta[2]) * oma + (ta[1] + ta[3]) * a)).sum(-1)
        sk = top * omb + bot * b
        ak = (ta[0] * oma + ta[1] * a) * omb + (ta[2] * oma + ta[3] * a) * b
        s0, a0 = np.where(at0[..., None], sk, s0), np.where(at0[..., None], ak, a0)
        s1, a1 = np.where(at1[..., None], sk, s1), np.where(at1[..., None], ak, a1)
    ma, m, su, sv = (np.asarray(fwd[k], np.float64) for k in ("ma", "m", "su", "sv"))
    hu, hv = 0.5 * gu, 0.5 * gv
    g_m = -((hu * su + hv * sv) / m)
    g_ma = np.where(ma < 0, -g_m, g_m)
    gd = cc._to_xyz(fwd["face"], hu / m, hv / m, g_ma, True)
    ad = cc._to_xyz(fwd["face"], 0.5 * au / m, 0.5 * av / m, (0.5 * au * np.abs(su) + 0.5 * av * np.abs(sv)) / m, False)
    passes = fwd["passes"] & fwd["above"] & lod_given
    gl = np.where(passes, (g * (s1 - s0)).sum(-1), 0.0)
    al = np.where(passes, (np.abs(g) * (a1 + a0)).sum(-1), 0.0)
    out = {"grad_packed": pack(gp), "n": pack(n), "S": pack(S), "grad_directions": np.where(v[..., None], gd, 0.0),
           "abs_directions": np.where(v[..., None], ad, 0.0), "grad_lod": gl, "abs_lod": al}
    if shared:
        out.update({k: out[k][0] for k in ("grad_packed", "n", "S")})
    return out


# ---- bounds (U = 2^-24, the unit roundoff of float32), each k counted from the kernels' lines
#
# grad_packed.  A term g * w1 * w2 * wl is three float32 products (texture_mip_cases.K_PACKED), a corner tap's term one
# more, by third: k = 4 roundings at most.  n terms take n - 1 additions in any order and grouping (the LDS patch and
# its flush regroup them, no more), each rounding a partial sum of at most S; the n-th unit absorbs the second order.
K_PACKED = tmc.K_PACKED + 1


def packed_bound(vjp):
    return (vjp["n"] + K_PACKED) * U * vjp["S"]


def directions_roundings(C):
    """Per level (gu, gv) are tex_grad_uv's lines: texture_cases.uv_roundings(C) = C + 5 units.  A corner tap's value
    adds its mean's three roundings (two sums, the product by third) under them, relative to the mean's own terms,
    which is what abs_directions holds for such pixels: C + 8.  The level blend is one product per level and one sum
    (texture_mip_cases.uv_bound's + 2): C + 10.  Then cubemap_cases.directions_roundings' chain from (gu, gv) to the
    direction: + 3.  C + 13 serves the three components; pixels without a corner, or with f == 0, stay below it."""
    return tc.uv_roundings(C) + 3 + 2 + 3


def directions_bound(vjp, C):
    return directions_roundings(C) * U * vjp["abs_directions"]


def lod_roundings(C):
    """grad_lod = sum_c g_c * (s_k1,c - s_k0,c).  A tap value reaches s_k through a product and a sum (top or bot) and
    a product and a sum again: 4 roundings, 3 more under them where the tap is a corner's mean.  The difference of the
    two levels is one, the product with g one, the C terms take C - 1 additions, and one unit absorbs the second
    order: 7 + 1 + 1 + (C - 1) + 1 = C + 9 units of sum_c |g_c| * (S_k1,c + S_k0,c), S_k the same bilinear blend of the
    absolute tap values (abs_lod)."""
    return C + 9


def lod_bound(vjp, C):
    return lod_roundings(C) * U * vjp["abs_lod"]


def cubemap_bound(vjp, S, levels=None):
    """texture_mip_cases.texture_bound per face with this file's K_PACKED: the chain's backward multiplies by 0.25
    exactly and adds L - 1 times; sum_k W_k (n_k + K_PACKED + L) U S_k over the levels above an element."""
    dims, _, _ = tmc.layout(S, S, levels)
    L = len(dims)
    per_level = (vjp["n"] + K_PACKED + L) * U * vjp["S"]
    scaled = [W * lv for W, lv in zip(tmc.chain_weights(S, S, levels), tmc.unpack(per_level, S, S, levels))]
    i, j = np.arange(S)[:, None], np.arange(S)[None, :]
    return sum(lv[..., i >> k, j >> k, :] for k, lv in enumerate(scaled))


def chain_vjp(grad_packed, S, levels=None):
    """grad_packed [..,6,N,C] -> grad_cubemap [..,6,S,S,C] (texture_mip_cases.chain_vjp, a face a frame)"""
    return tmc.chain_vjp(grad_packed, S, S, levels)


# ---- the table

def _d_seam_walk(shape, S, rng):
    """a smooth sweep across the +x / +z seam and the (+x, +y, +z) corner at about S / 32 texels per pixel, so that
    neighbouring pixels lie on different faces"""
    y, x = tc._yx(shape)
    a = (x - shape[2] / 2.0 + 0.3) * 0.06
    b = (y - shape[1] / 2.0 + 0.3) * 0.06
    return np.stack([1.0 + a, 1.0 + b * 0.5 - np.abs(a) * 0.2, 1.0 - a + b], -1)


PATTERNS = dict(cc.PATTERNS, **{"seam-walk": _d_seam_walk})


# (id, frame, S, C, per-frame chain, pattern, holes, lod mode, lod_bias, seamless)
# holes as cubemap_cases; lod mode: "auto"; "int" (an explicit integer-valued lod over -1 .. L, with a NaN); "frac" (an
# explicit fractional lod beyond both ends of the chain, with an inf and a NaN)
def _table():
    rows = []

    def add(frame, S, C, per_frame, pattern, holes=None, mode="auto", bias=0.0, seamless=True):
        ident = "%s-s%d-c%d-%s-%s-%s%s%s%s" % (frame, S, C, "perframe" if per_frame else "shared", pattern, mode,
                                              "-" + holes if holes else "", "-bias%+.2f" % bias if bias else "",
                                              "" if seamless else "-clamped")
        rows.append((ident, frame, S, C, per_frame, pattern, holes, mode, bias, seamless))

    # every frame x every size, everything else cycling
    k = 0
    for frame in FRAMES:
        for S in SIZES:
            add(frame, S, (1, 3, 4, 8)[k % 4], frame == "3x5x6" and k % 2 == 1, "random", (None, "bg", "mask")[k % 3],
                ("auto", "frac", "int")[k % 3], (0.0, 0.0, 0.0, 0.7, -0.6)[k % 5], k % 7 != 3)
            k += 1
    # every channel count the kernels are compiled for, under every way a tile is summed and every branch of the lod
    for C in range(1, 9):
        add("17x33", 64, C, False, "oneface-magnify", "bg")                      # one face's box, an empty tile
        add("17x33", 64, C, False, "oneface-magnify", "bg", "frac", -4.5)        # the boxes of two levels
        add("17x33", 64, C, False, "corner", "bg" if C % 2 else None, "frac")    # seams: memory below S_k = 8
        add("17x33", 8, C, C % 2 == 0, "random", "mask", "int")                  # whole levels; corners at S_k = 1
        add("3x5x6", 64, C, True, "seam-walk", "mask", "auto", 0.0 if C % 2 else 1.5)
        add("17x33", 64, C, False, "seam-walk", "bg")
    for S in (1, 2, 5, 8):
        add("15x17", S, 3, False, "lattice", None, "frac")
        add("15x17", S, 3, False, "lattice", None, "frac", 0.0, False)
    add("16x16", 64, 3, False, "oneface-scatter", None, "int")
    add("16x16", 64, 4, False, "corner", None, "auto", 2.0)
    add("17x33", 64, 3, False, "corner", "bg", "frac", 0.0, False)
    return rows


TABLE = _table()
CASE_IDS = [r[0] for r in TABLE]
assert len(set(CASE_IDS)) == len(CASE_IDS)
_ROWS = {r[0]: r for r in TABLE}


@functools.lru_cache(maxsize=None)
def case_input(ident):
    """dict: cubemap float32 ([6,S,S,C] or [B,6,S,S,C]), directions float32 [B,H,W,3], mask uint8 [B,H,W] or None, lod
    float32 [B,H,W] or None, lod_bias, seamless, grad float32 [B,H,W,C]"""
    _, frame, S, C, per_frame, pattern, holes, mode, bias, seamless = _ROWS[ident]
    shape = FRAMES[frame]
    rng = tc._rng(ident)
    cubemap = rng.standard_normal(((shape[0],) if per_frame else ()) + (6, S, S, C)).astype(F32)
    d = np.ascontiguousarray(PATTERNS[pattern](shape, S, rng), F32)
    mask = None
    if holes:
        d[rng.random(shape) < 0.25] = -np.inf
        if shape[2] >= 32:
            d[:, :16, 16:32] = -np.inf  # a tile with no sampled pixel
        flat = d.reshape(-1, 3)
        if len(flat) >= 8:
            flat[1, 0] = np.nan
            flat[3] = 0.0
        if shape[1] >= 8 and shape[2] >= 8:  # a sampled pixel with no sampled neighbour, one with previous ones only
            d[:, 4:7, 4:7] = -np.inf
            d[:, 5, 5] = (0.3, -0.2, 1.0)
            d[:, 9:12, 9:12] = -np.inf
            d[:, 10, 10] = d[:, 10, 9] = d[:, 9, 10] = (0.25, 1.0, -0.5)
        if holes == "mask":
            mask = (rng.random(shape) < 0.7).astype(np.uint8)
            if len(flat) >= 8:
                mask.reshape(-1)[[1, 3]] = 1  # set over the NaN and the zero vector
    L = len(tmc.layout(S, S)[0])
    lod = None
    if mode == "int":
        lod = rng.integers(-1, L + 1, shape).astype(F32)
        lod.reshape(-1)[0] = np.nan
    elif mode == "frac":
        lod = rng.uniform(-0.5, L - 0.5, shape).astype(F32)
        lod.reshape(-1)[-1] = np.inf
        lod.reshape(-1)[0] = np.nan
    grad = rng.standard_normal(shape + (C,)).astype(F32)
    return dict(cubemap=cubemap, directions=d, mask=mask, lod=lod, lod_bias=bias, seamless=seamless, grad=grad)


def statement(inp, dtype=F32):
    """(chain, forward dict, vjp dict with grad_cubemap and its bound besides) of the statement for case_input's dict"""
    chain = build_chain(inp["cubemap"], None, dtype)
    fwd = sample(chain, inp["directions"], inp["mask"], inp["lod"], inp["lod_bias"], inp["seamless"], dtype)
    vjp = sample_vjp(chain, inp["grad"], fwd, inp["lod"] is not None)
    S = inp["cubemap"].shape[-2]
    vjp["grad_cubemap"] = chain_vjp(vjp["grad_packed"], S)
    vjp["cubemap_bound"] = cubemap_bound(vjp, S)
    return chain, fwd, vjp


@functools.lru_cache(maxsize=None)
def case(ident):
    """(inputs, chain, forward dict, vjp dict) of the float32 statement: computed once per process, read-only"""
    inp = case_input(ident)
    return (inp,) + statement(inp)


# ---- how the backward treats a 16 x 16 screen tile, from the statement's taps alone (the kernels are not consulted).
# The tile's lowest k0 is level A, the one above it B.  Per level, over the lanes with taps there (A: k0 = A; B: the
# second level of those that blend, and the first of the lanes with k0 = B): `whole` when the level's whole cube,
# 6 * T^2 texels, fits what is left of the LDS budget; else `box` when those lanes lie on one face, every tap in range,
# and the box of their taps fits; else `memory`.  A is served first.  The budget is DIRT_CUBEMAP_MIP_PATCH of
# dirt_amd/csrc/cubemap_mip_kernels.h, restated here: a changed kernel budget is a table change.
PATCH_TEXELS = 1408
DISPOSITIONS = ("whole", "box", "memory", "empty")  # (a tile counts under each way one of its two levels is summed)
EXTRAS = ("above",)  # a tile with LDS in use and a lane two or more levels above A (its taps go to memory)


def _plan(lanes, lv, face, budget):
    """-> (mode, texels of LDS) of one level of a tile (lv: level_sample's dict cut to the tile)"""
    if not lanes.any():
        return None, 0
    T = lv["T"]
    if 6 * T * T <= budget:
        return "whole", 6 * T * T
    box = tc.tap_box(lanes, lv["r0"], lv["r1"], lv["c0"], lv["c1"])
    one_face = len(set(face[lanes].tolist())) == 1
    in_range = box[0] >= 0 and box[1] >= 0 and box[0] + box[2] <= T and box[1] + box[3] <= T
    if one_face and in_range and box[2] * box[3] <= budget:
        return "box", box[2] * box[3]
    return "memory", 0


def dispositions(fwd, budget=PATCH_TEXELS):
    """-> {disposition or extra: tiles} of one forward dict"""
    n = dict.fromkeys(DISPOSITIONS + EXTRAS, 0)
    cut = lambda lv, sl: {k: (a[sl] if isinstance(a, np.ndarray) else a) for k, a in lv.items()  # noqa: E731
                          if k in ("T", "r0", "r1", "c0", "c1")}
    for sl in tc.tiles(fwd["valid"].shape):
        v, k0, blend, face = fwd["valid"][sl], fwd["k0"][sl], fwd["blend"][sl], fwd["face"][sl]
        if not v.any():
            n["empty"] += 1
            continue
        kA = int(k0[v].min())
        hasA, firstB = v & (k0 == kA), v & (k0 == kA + 1)
        hasB = firstB | (hasA & blend)
        mA, usedA = _plan(hasA, cut(fwd["levels"][kA], sl), face, budget)
        mB, usedB = _plan(hasB, cut(fwd["levels"][kA + 1], sl), face, budget - usedA) if hasB.any() else (None, 0)
        for mode in {mA, mB} - {None}:
            n[mode] += 1
        if usedA + usedB and (v & (k0 >= kA + 2)).any():
            n["above"] += 1
    return n


def coverage_counts():
    """-> {C: {condition: pixels or tiles}} over the table"""
    out = {}
    for row in TABLE:
        _, _, fwd, _ = case(row[0])
        per_c = out.setdefault(row[3], {})
        v, L = fwd["valid"], len(tmc.layout(row[2], row[2])[0])
        kinds = [np.zeros(v.shape, np.int64)]
        for k, lv in fwd["levels"].items():
            reads = v & ((fwd["k0"] == k) | (fwd["blend"] & (fwd["k1"] == k)))
            kinds.append(np.where(reads, np.max(lv["kind"], 0), 0))
        worst = np.max(kinds, 0)
        got = dict(dispositions(fwd))
        got.update(folded=int(np.any([(np.asarray(lv["kind"]) == 1).any(0) & lv["sel"] for lv in
                                      fwd["levels"].values()], 0).sum()) if fwd["levels"] else 0,
                   corner=int((worst == 2).sum()),
                   f_zero_below_top=int((v & (fwd["f"] == 0) & (fwd["k0"] < L - 1) & (L > 1)).sum()),
                   f_frac=int((v & (fwd["f"] > 0) & (fwd["f"] < 1)).sum()),
                   clamped_low=int((v & (fwd["raw"] < 0)).sum()), clamped_high=int((v & (fwd["raw"] > L - 1)).sum()),
                   nan_lod=int(fwd["nan"].sum()))
        if row[7] == "auto":
            for name, br in (("next", 0), ("previous", 1), ("none", 2)):
                got["auto_" + name] = int((v & ((fwd["branch_x"] == br) | (fwd["branch_y"] == br))).sum())
            got["auto_other_face"] = int(fwd["other_face"].sum())
        for k, val in got.items():
            per_c[k] = per_c.get(k, 0) + val
    return out


CONDITIONS = DISPOSITIONS + ("folded", "corner", "f_zero_below_top", "f_frac", "clamped_low", "clamped_high", "nan_lod",
                             "auto_next", "auto_previous", "auto_none", "auto_other_face")


def _coverage():
    counts = coverage_counts()
    for C in range(1, 9):
        assert C in counts and all(counts[C].get(k, 0) > 0 for k in CONDITIONS), \
            (C, {k: counts.get(C, {}).get(k, 0) for k in CONDITIONS})
    assert any(n.get("above", 0) for n in counts.values()), counts


_coverage()


# ---- the exact scatter: every coordinate on a half texel of the levels it reads, f in {0, 1/2}, |ma| = 1, small
# integer cotangents and texels (times 64: three levels of box means stay integers): every product and partial sum of
# the three gradients is exact in float32, whatever the order of the atomics.  No pixel has a corner tap (third is
# not a dyadic number); folded taps are in.

@functools.lru_cache(maxsize=None)
def exact_scatter_case(kind, C=3, frames=1):
    """kind 'box': one texel step every 16 pixels on the +z face, lod in {0, 1/2, 1} (the boxes of two levels);
    'memory': random positions on random faces, lod in {0, .., 3}; 'whole': those positions with lod in {2, 5/2, 3}
    (level 3, 6 * 8 * 8 texels, as a whole; level 2 beside it in memory).  The chain is shared: with frames > 1 its
    gradient sums over them.  -> (inputs, chain, forward dict, vjp dict)"""
    shape, S = (frames, 33, 35), 64
    rng = tc._rng("cubemipexact", kind, C, frames)
    if kind == "box":
        y, x = tc._yx(shape)
        ku, kv, face = 5 + (x // 16).astype(np.int64), 9 + (y // 16).astype(np.int64), 4
        lod = rng.integers(0, 3, shape) / 2.0
    else:
        # u = k / 16: x_k = 64 u / 2^k - 0.5 = 4 k / 2^k - 0.5 has fraction 1/2 at the levels 0..2, 0 or 1/2 at level 3;
        # ku = 0 puts u on a face's edge (a folded tap of weight 1/2); kv in 3..13 stays inside at every level read,
        # mirrored or not: no corner
        ku, kv, face = rng.integers(0, 15, shape), rng.integers(3, 14, shape), rng.integers(0, 6, shape)
        lod = (rng.integers(0, 7, shape) if kind == "memory" else rng.integers(4, 7, shape)) / 2.0
    d = cc.on_face(face, ku / 16.0, kv / 16.0).astype(F32)
    d[:, 3, 4] = -np.inf
    cubemap = rng.integers(-2, 3, (6, S, S, C)).astype(F32) * 64.0
    grad = rng.integers(-3, 4, shape + (C,)).astype(F32)
    inp = dict(cubemap=cubemap, directions=d, mask=None, lod=lod.astype(F32), lod_bias=0.0, seamless=True, grad=grad)
    chain, fwd, vjp = statement(inp)
    for k, lv in fwd["levels"].items():
        # (level 4 is read by the lod's gradient alone, at lod 3 exactly: quarter weights there, dyadic still)
        assert set(np.unique(lv["a"])) | set(np.unique(lv["b"])) <= ({0.0, 0.5} if k <= 3 else {0.0, 0.25, 0.5, 0.75})
        assert not np.any([(kd == 2) & lv["sel"] for kd in lv["kind"]])
    assert set(np.unique(fwd["f"])) == {0.0, 0.5} and np.array_equal(fwd["m"], np.ones_like(fwd["m"]))
    disp = dispositions(fwd)
    assert disp[kind] > 0, (kind, disp)
    if kind != "box":
        assert any(((np.asarray(lv["kind"]) == 1).any(0) & lv["sel"]).any() for lv in fwd["levels"].values())
    return inp, chain, fwd, vjp


# ---- continuity: a smooth function on the sphere, sampled at the texel centres of every level, and pairs of
# directions that straddle each of the 12 seams and the 8 corners

def smooth_function(d):
    """[..,3] directions -> [..,2] values of a smooth function of the unit direction"""
    n = d / np.linalg.norm(d, axis=-1, keepdims=True)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return np.stack([0.5 + 0.4 * x - 0.3 * y * z + 0.2 * z, np.sin(1.3 * x + 0.7 * y) + 0.5 * z * z], -1)


def smooth_chain(S):
    """the chain whose every level holds smooth_function at its own texel centres (float32)"""
    chain = []
    for (T, _) in tmc.layout(S, S)[0]:
        c = (np.arange(T) + 0.5) / T
        v, u = np.meshgrid(c, c, indexing="ij")
        faces = np.stack([smooth_function(cc.on_face(face, u, v)) for face in range(6)])
        chain.append(faces.astype(F32))
    return chain


def straddling_pairs(eps=1e-6, per_seam=5):
    """-> (first, second [n,3] float32, corner [n] bool): pairs of directions a relative eps apart, the two of a pair
    on different faces: per_seam pairs along each of the 12 seams, and 3 pairs around each of the 8 corners"""
    first, second, corner = [], [], []
    signs = (-1.0, 1.0)
    for ax in range(3):              # the seam between the faces of axes a and b, at sign sa, sb; c runs along it
        a, b = [k for k in range(3) if k != ax]
        for sa in signs:
            for sb in signs:
                for c in np.linspace(-0.8, 0.8, per_seam):
                    p, q = np.zeros(3), np.zeros(3)
                    p[a], p[b], p[ax] = sa, sb * (1 - eps), c + 0.013
                    q[a], q[b], q[ax] = sa * (1 - eps), sb, c + 0.013
                    first.append(p), second.append(q), corner.append(False)
    for sx in signs:
        for sy in signs:
            for sz in signs:
                s = np.array([sx, sy, sz])
                for k in range(3):
                    p, q = s.copy(), s.copy()
                    p[(k + 1) % 3] *= 1 - eps
                    p[(k + 2) % 3] *= 1 - 2 * eps
                    q[k] *= 1 - eps
                    q[(k + 2) % 3] *= 1 - 2 * eps
                    first.append(p), second.append(q), corner.append(True)
    return np.array(first, F32), np.array(second, F32), np.array(corner)
