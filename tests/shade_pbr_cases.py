"""Statement of record for deferred.shade_pbr (dirt_amd/deferred.py, dirt_amd/csrc/shade_pbr_kernels.h): numpy
float64, no torch and no code shared with either implementation.  TEST INFRASTRUCTURE ONLY.

Dilation of positions and normals under the positions' background, `valid` and the route word are
tests/deferred_cases.py's; colours, material and visibility are read at the pixel itself.  For a valid pixel with
dilated position p, dilated normal n_d, colour c, material (r_0, m_0), u(x) = x / (|x| + 1e-12), in this order:
    n = u(n_d)   v = u(cam - p)   l = u(-d_i) (directional) or u(q_i - p) (point)   h = u(l + v)
    r = clamp(r_0, R_MIN, 1)   m = clamp(m_0, 0, 1)   alpha = r r   k = alpha / 2
    nl = n . l   nv = max(n . v, 0)   nh = n . h   vh = clamp(v . h, 0, 1)
    x = n x h   t = x . x + (nh alpha)^2   D = t > 0 ? alpha^2 / (pi t^2) : 0
    gl = nl (1 - k) + k   gv = nv (1 - k) + k   V = 1 / (4 (gl gv))
    F0 = 0.04 + (c - 0.04) m   w = 1 - vh   w5 = ((w w) (w w)) w   F = F0 + (1 - F0) w5
    d_i = (lc_i nl) (((1 - F) (1 - m)) c / pi)   s_i = (lc_i nl) ((D V) F)
    term_i = nl > 0 ? vis_i (d_i + s_i) : 0
    acc = term_0;  acc = acc + term_i;  pixels = acc + c * ambient
Invalid pixels are exactly 0.  Every clamp takes torch.clamp's derivative (the gradient passes where min <= x <= max,
ends included); u's subgradient at 0 is 0 (lighting_f64's rule); the two selects (nl > 0, t > 0) pass no gradient on
their zero side.

Gradients, derived by hand in `light_rows` (checked against central differences by tests/test_shade_pbr_cpu.py): the
adjoints of the dilated position and normal are routed through the dilation by deferred_cases.gather; colours, material
and visibility receive their own pixel's terms; a parameter's gradient is the sum of its per-pixel terms over the valid
pixels of its frame (per-frame parameters) or of all frames (shared ones).  `absum` is, per parameter element, the sum
over the pixels (and, for the camera, over the lights) of the absolute per-pixel terms: the scale a float32 sum of those
terms is judged by.  `scale` = |c * ambient| + sum_i (|d_i| + |s_i|) over the lights with nl > 0.
"""
import functools

import numpy as np

import deferred_cases as dc
import lighting_f64 as lf
from deferred_cases import FRAMES  # noqa: F401
from shade_lights_cases import KINDS, param_ratio  # noqa: F401  (the light kinds and the parameter comparison, reused)

F32 = np.float32
MAX_LIGHTS = 8
R_MIN = float(F32(0.045))
PARAMS = ("vectors", "colors", "camera", "ambient")
PIXEL_NAMES = ("positions", "colors", "normals", "material", "visibility")


def _clamp_pass(x, lo, hi):
    """torch.clamp's derivative: 1 where lo <= x <= hi"""
    return ((x >= lo) & (x <= hi)).astype(np.float64)


@lf._quiet
def light_rows(p, nd, c, mat, vis, g, vector, lc, cam, point):
    """One light on rows: p, nd, c [R,3], mat [R,2], vis [R,1], g [R,3] or None, vector, lc, cam [3] (float64).
    -> dict: d, s (the two terms without the visibility, zero where nl <= 0), term; with g every per-row adjoint:
    positions, normals (of the dilated values), colors, material [R,2], visibility [R,1], and the per-row parameter
    terms vectors, light_colors, camera [R,3]."""
    vector, lc, cam = lf._f64(vector), lf._f64(lc), lf._f64(cam)
    n = lf._over_length_eps(nd)
    tc = cam - p
    v = lf._over_length_eps(tc)
    lraw = (vector - p) if point else np.broadcast_to(-vector, p.shape)
    l = lf._over_length_eps(lraw)
    hs = l + v
    h = lf._over_length_eps(hs)
    r0, m0 = mat[:, 0:1], mat[:, 1:2]
    r = np.minimum(np.maximum(r0, R_MIN), 1.0)
    m = np.minimum(np.maximum(m0, 0.0), 1.0)
    al = r * r
    k = al / 2.0
    nl = lf._dot(n, l)
    nvr = lf._dot(n, v)
    nv = np.maximum(nvr, 0.0)
    nh = lf._dot(n, h)
    vhr = lf._dot(v, h)
    vh = np.minimum(np.maximum(vhr, 0.0), 1.0)
    x = np.cross(n, h)
    a = nh * al
    t = lf._dot(x, x) + a * a
    pos_t = t > 0
    ts = np.where(pos_t, t, 1.0)
    D = np.where(pos_t, al * al / (np.pi * ts * ts), 0.0)
    lit = nl > 0
    nls = np.where(lit, nl, 1.0)  # (the unlit side is a select: nothing of it is used)
    omk = 1.0 - k
    gl = nls * omk + k
    gv = nv * omk + k
    V = 1.0 / (4.0 * (gl * gv))
    F0 = 0.04 + (c - 0.04) * m
    w = 1.0 - vh
    w2 = w * w
    w4 = w2 * w2
    w5 = w4 * w
    F = F0 + (1.0 - F0) * w5
    om = 1.0 - m
    dd = ((1.0 - F) * om) * c / np.pi
    e = lc * nls
    DV = D * V
    d = np.where(lit, e * dd, 0.0)
    s = np.where(lit, e * (DV * F), 0.0)
    out = {"d": d, "s": s, "term": vis * (d + s)}
    if g is None:
        return out
    Bc = dd + DV * F
    g = np.where(lit, g, 0.0)
    out["visibility"] = lf._dot(g, e * Bc)
    gt = g * vis
    g_lc = gt * nls * Bc
    g_nl = lf._dot(gt * lc, Bc)
    gB = gt * e
    g_DV = lf._dot(gB, F)
    g_F = gB * (DV - om * c / np.pi)
    g_m = -lf._dot(gB, (1.0 - F) * c / np.pi)
    g_c = gB * ((1.0 - F) * om / np.pi)
    g_F0 = g_F * (1.0 - w5)
    g_w5 = lf._dot(g_F, 1.0 - F0)
    g_c = g_c + g_F0 * m
    g_m = g_m + lf._dot(g_F0, c - 0.04)
    g_vhr = -(g_w5 * 5.0 * w4) * _clamp_pass(vhr, 0.0, 1.0)
    g_D, g_V = g_DV * V, g_DV * D
    g_gl, g_gv = -g_V * V / gl, -g_V * V / gv
    g_nl = g_nl + g_gl * omk
    g_nvr = g_gv * omk * (nvr >= 0)
    g_k = g_gl + g_gv - (g_gl * nls + g_gv * nv)
    g_al = g_k / 2.0
    g_al = g_al + np.where(pos_t, g_D * 2.0 * D / al, 0.0)
    g_t = np.where(pos_t, -2.0 * D / ts * g_D, 0.0)
    g_x = 2.0 * x * g_t
    g_a = 2.0 * a * g_t
    g_nh = g_a * al
    g_al = g_al + g_a * nh
    g_n = np.cross(h, g_x) + g_nh * h + g_nvr * v + g_nl * l
    g_h = np.cross(g_x, n) + g_nh * n + g_vhr * v
    g_v = g_vhr * h + g_nvr * n
    g_l = g_nl * n
    g_hs = lf._over_length_eps_vjp(hs, g_h)
    g_l = g_l + g_hs
    g_v = g_v + g_hs
    g_lraw = lf._over_length_eps_vjp(lraw, g_l)
    g_tc = lf._over_length_eps_vjp(tc, g_v)
    g_p = -g_tc
    if point:
        g_p = g_p - g_lraw
        g_vec = g_lraw
    else:
        g_vec = -g_lraw
    g_r = 2.0 * r * g_al
    out.update({"positions": g_p, "normals": lf._over_length_eps_vjp(nd, g_n), "colors": g_c,
                "material": np.concatenate([g_r * _clamp_pass(r0, R_MIN, 1.0), g_m * _clamp_pass(m0, 0.0, 1.0)], -1),
                "vectors": g_vec, "light_colors": g_lc, "camera": g_tc})
    return out


# ---- the parameters of one call

class LightSet:
    """float32 values, as both implementations receive them: vectors, colors [N,3] or [B,N,3]; camera [3] or [B,3];
    ambient [3] or None; point a tuple of N bools."""

    def __init__(self, vectors, colors, camera, ambient, point):
        self.vectors, self.colors = (np.asarray(x, F32) for x in (vectors, colors))
        self.camera = np.asarray(camera, F32)
        self.ambient = None if ambient is None else np.asarray(ambient, F32)
        self.point = tuple(bool(b) for b in point)
        self.n = self.vectors.shape[-2]
        assert len(self.point) == self.n <= MAX_LIGHTS

    def frame(self, b):
        """(vectors [N,3], colors [N,3], camera [3]) of frame b"""
        pick = lambda a, d: a[b] if a.ndim == d else a  # noqa: E731
        return pick(self.vectors, 3), pick(self.colors, 3), pick(self.camera, 2)


def draw_lights(rng, frames, n=2, kinds="mixed", per_frame=False, ambient=True):
    """Lights as shade_lights_cases.draw_lights draws them, for positions in [-1, 1]^3: directions of length 0.8 .. 1,
    point positions 2.3 .. 3 from the origin (at least 0.5 from every position), colours in [0.1, 1]; per_frame: one
    set and one camera (near deferred_cases.Lights().camera) per frame."""
    lead = (frames,) if per_frame else ()
    point = tuple(KINDS[kinds](i) for i in range(n))
    unit = rng.standard_normal(lead + (n, 3))
    unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
    radius = np.where(np.asarray(point, bool)[:, None], rng.uniform(2.3, 3.0, lead + (n, 1)),
                      rng.uniform(0.8, 1.0, lead + (n, 1)))
    vectors = (unit * radius).astype(F32)
    colors = rng.uniform(0.1, 1.0, lead + (n, 3)).astype(F32)
    camera = (np.asarray(dc.Lights().camera, np.float64) + (rng.uniform(-0.2, 0.2, lead + (3,)) if per_frame else 0.0))
    amb = rng.uniform(0.1, 1.0, 3).astype(F32) if ambient else None
    return LightSet(vectors, colors, camera, amb, point)


def random_input(rng, covered, n_lights, invalid=None, roughness=(0.2, 1.0)):
    """(positions, colors, normals, material, visibility) float32 over `covered` [B,H,W] bool: unit normals, positions
    in [-1, 1]^3, colours in [0.2, 1], -inf background in positions and normals; roughness in `roughness`, metallic in
    [0, 1] and visibility [B,H,W,N] in [0, 1] everywhere; `invalid` marks covered pixels whose normal is NaN."""
    shape = covered.shape + (3,)
    n = rng.standard_normal(shape)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    p = rng.uniform(-1.0, 1.0, shape).astype(F32)
    c = rng.uniform(0.2, 1.0, shape).astype(F32)
    mat = np.stack([rng.uniform(roughness[0], roughness[1], covered.shape), rng.uniform(0.0, 1.0, covered.shape)],
                   -1).astype(F32)
    vis = rng.uniform(0.0, 1.0, covered.shape + (n_lights,)).astype(F32)
    p[~covered] = -np.inf
    n[~covered] = -np.inf
    if invalid is not None:
        n[invalid & covered] = np.nan
    return p, c, n, mat, vis


# ---- the statement

def shade_pbr(positions, colors, normals, material, visibility, L, grad=None):
    """-> dict: pixels (float64), valid (bool [B,H,W]), route (uint32), scale (for the forward bound); with grad also
    the per-pixel gradients positions / colors / normals / material / visibility, `params` {name: gradient, shaped as
    the parameter (ambient None: absent)} and `absum` (same shapes).  visibility None is ones.  [H,W,.] inputs give
    unbatched results."""
    squeeze, rp, rn, valid, P, N, C = dc._shade_terms(positions, colors, normals, None)
    B, H, W = valid.shape
    M = np.asarray(dc._batched(material)[0], np.float64)
    Vs = np.ones((B, H, W, L.n)) if visibility is None else np.asarray(dc._batched(visibility)[0], np.float64)
    pixels, scale = np.zeros(P.shape), np.zeros(P.shape)
    out = {"valid": valid,
           "route": (rp | (rn << np.uint32(12)) | (valid.astype(np.uint32) << np.uint32(31))).astype(np.uint32)}
    amb = np.zeros(3) if L.ambient is None else np.asarray(L.ambient, np.float64)
    if grad is not None:
        G = np.asarray(dc._batched(grad)[0], np.float64)
        a_pos, a_nrm, a_col = np.zeros(P.shape), np.zeros(P.shape), np.zeros(P.shape)
        a_mat, a_vis = np.zeros(M.shape), np.zeros(Vs.shape)
        shapes = {"vectors": L.vectors.shape, "colors": L.colors.shape, "camera": L.camera.shape, "ambient": (3,)}
        params = {k: np.zeros(s) for k, s in shapes.items()}
        absum = {k: np.zeros(s) for k, s in shapes.items()}
    for b in range(B):
        sel = valid[b]
        p, n, c, mat = P[b][sel], N[b][sel], C[b][sel], M[b][sel]
        g = None if grad is None else G[b][sel]
        vectors, lcs, cam = L.frame(b)
        acc, sc = np.zeros(p.shape), np.abs(c * amb)
        for i in range(L.n):
            vis = Vs[b][sel][:, i:i + 1]
            t = light_rows(p, n, c, mat, vis, g, vectors[i], lcs[i], cam, L.point[i])
            acc = t["term"] if i == 0 else acc + t["term"]
            sc = sc + np.abs(t["d"]) + np.abs(t["s"])
            if g is None:
                continue
            a_pos[b][sel] += t["positions"]
            a_nrm[b][sel] += t["normals"]
            a_col[b][sel] += t["colors"]
            a_mat[b][sel] += t["material"]
            col = np.zeros((int(sel.sum()), L.n))
            col[:, i:i + 1] = t["visibility"]
            a_vis[b][sel] += col
            for name, key in (("vectors", "vectors"), ("colors", "light_colors"), ("camera", "camera")):
                at = ((b,) if params[name].ndim == (3 if name != "camera" else 2) else ())
                if name != "camera":
                    at = at + (i,)
                params[name][at] += t[key].sum(0)
                absum[name][at] += np.abs(t[key]).sum(0)
        pixels[b][sel] = acc + c * amb
        scale[b][sel] = sc
        if g is not None:
            a_col[b][sel] += g * amb
            params["ambient"] += (g * c).sum(0)
            absum["ambient"] += np.abs(g * c).sum(0)
    out["pixels"], out["scale"] = pixels, scale
    if grad is not None:
        out["positions"] = dc.gather(a_pos, dc.codes(rp, 3))[0]
        out["normals"] = dc.gather(a_nrm, dc.codes(rn, 3))[0]
        out["colors"], out["material"], out["visibility"] = a_col, a_mat, a_vis
        if L.ambient is None:
            del params["ambient"], absum["ambient"]
        out["params"], out["absum"] = params, absum
    if squeeze:
        out = {k: (a if k in ("params", "absum") else a[0]) for k, a in out.items()}
    return out


def fwd_bound(ref, n):
    """The lighting contract (tests/lighting_cases.py) per term and summed: one ambient, n diffuse, n specular"""
    import lighting_cases
    return (1 + 2 * n) * lighting_cases.FWD_ATOL + lighting_cases.FWD_RTOL * ref["scale"]


# ---- references, computed once per process and shared by the tests (treat as read-only)

def light_set(ident, n=2, kinds="mixed", per_frame=False, ambient=True):
    """draw_lights for the frame `ident` of the table, seeded by its name"""
    L = draw_lights(dc._rng(ident, 31, n, len(kinds), int(per_frame)), dict(FRAMES)[ident].shape[0], n, kinds,
                    per_frame, ambient)
    positions = dc.shade_input(ident)[0]
    finite = positions[np.isfinite(positions).all(-1)].astype(np.float64)
    for v in L.vectors.reshape((-1, n, 3) if n else (0, 0, 3)):
        for i in range(n):
            if L.point[i] and len(finite):
                assert np.linalg.norm(finite - v[i], axis=-1).min() >= 0.5
    return L


def frame_input(ident, n, roughness=(0.2, 1.0)):
    """deferred_cases.shade_input's G-buffers with a material and a visibility drawn for them"""
    p, c, nrm = dc.shade_input(ident)
    rng = dc._rng(ident, 32, n, int(round(roughness[0] * 1000)))
    shape = p.shape[:-1]
    mat = np.stack([rng.uniform(roughness[0], roughness[1], shape), rng.uniform(0.0, 1.0, shape)], -1).astype(F32)
    vis = rng.uniform(0.0, 1.0, shape + (n,)).astype(F32)
    return p, c, nrm, mat, vis


@functools.lru_cache(maxsize=None)
def case(ident, n=2, kinds="mixed", per_frame=False, ambient=True, roughness=(0.2, 1.0)):
    """(inputs (positions, colors, normals, material, visibility), LightSet, upstream gradient float32, statement dict
    with gradients) for one frame of the table"""
    inputs = frame_input(ident, n, roughness)
    L = light_set(ident, n, kinds, per_frame, ambient)
    grad = dc._rng(ident, 9).standard_normal(inputs[0].shape).astype(F32)
    return inputs, L, grad, shade_pbr(*inputs, L, grad)


def accuracy_frames():
    """the frames whose parameter gradients are held to GRAD_FRAC * absum: all but those with a single valid pixel
    (one pixel's terms may cancel within themselves, as shade_lights_cases.accuracy_frames has it)"""
    return [i for i in dc.FRAME_IDS if not i.startswith("1x1-")]
