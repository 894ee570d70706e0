"""Statement of record for deferred.shade_lights (dirt_amd/deferred.py, dirt_amd/csrc/shade_lights_kernels.h): numpy
float64, no torch and no code shared with either implementation.  TEST INFRASTRUCTURE ONLY.

Dilation, `valid` and the route word are tests/deferred_cases.py's.  For a valid pixel, the lights in index order:
    acc = (d_0 + s_0);  acc = acc + (d_i + s_i);  pixels = acc + colors * ambient
  directional light (row l of `vectors`, used raw): d_i = lighting_f64.diffuse_directional, s_i =
    lighting_f64.specular_directional, the colours as reflectivities;
  point light (row = its position): u = (p - light) / (|p - light| + eps), d_i = lighting_f64.diffuse_point, s_i =
    `specular_point` below: specular_directional with u in place of the light direction, no attenuation.

Gradients: the G-buffer adjoints of the lights are summed and routed through the dilation by deferred_cases.gather;
a parameter's gradient is the sum of its per-pixel terms over the valid pixels of its frame (per-frame parameters) or
of all frames (shared ones).  The gradients of the three existing helpers come from lighting_f64's `_vjp` functions;
`specular_point_vjp` is derived here (checked against central differences by tests/test_shade_lights_cpu.py):
  with u = rel / (|rel| + eps), rel = p - light, and the directional statement's g_refl, n_gr for direction u,
    g_u = g_refl - 2 n_gr n                 (reflected = u + 2 (n . (-u)) n)
    g_rel = J^T g_u,  J = I / d - h h^T |rel| / d^2,  d = |rel| + eps, h = rel / |rel|   (lighting_f64's rule)
    positions += g_rel,   light_position = -sum g_rel
  the camera, the normal's other terms, the reflectivity, light_color and the shininess as for a directional light.
`absum` is, per parameter element, the sum over the pixels of the absolute per-pixel terms (`_light_rows`, which
restates every term per pixel; its sums are held to the `_vjp` functions by the same test): the scale a float32 sum of
those terms is judged by.
"""
import functools

import numpy as np

import deferred_cases as dc
import lighting_f64 as lf
from deferred_cases import FRAMES, shade_input  # noqa: F401  (the frame table and its G-buffers, reused)

F32 = np.float32
MAX_LIGHTS = 8
PARAMS = ("vectors", "diffuse", "specular", "camera", "ambient", "shininess")


# ---- the point light's specular term

def _per_row_specular(p, n, r, l, lc, cam, k, two, g=None):
    """specular_directional with one light direction per row (l [R,3]); with g: every per-row term of its vjp."""
    p, n, r, l = (lf._f64(x) for x in (p, n, r, l))
    lc, cam = lf._f64(lc), lf._f64(cam)
    to_light, reflected, to_cam, view = lf._spec_terms(p, n, l, cam)
    cos = lf._dot(view, reflected)
    cs = lf._clamp(cos, two)
    pw = lf._power(cs, k)
    out = lc * r * pw
    if g is None:
        return out
    g = lf._f64(g)
    g_pw = lf._dot(g, lc * r)
    with np.errstate(invalid="ignore", divide="ignore"):
        g_cos = lf._clamp_vjp(cos, g_pw * lf._power_slope(cs, k), two)
        g_view, g_refl = g_cos * reflected, g_cos * view
        tl = lf._length(to_cam)
        h = to_cam / tl
        g_to_cam = (g_view - h * lf._dot(h, g_view)) / tl
        g_k = g_pw * np.where(cs > 0, pw * np.log(np.where(cs > 0, cs, 1.0)), np.where(cs == 0, 0.0, np.nan))
    s, n_gr = lf._dot(n, to_light), lf._dot(n, g_refl)
    return {"out": out, "positions": -g_to_cam, "normals": 2.0 * s * g_refl + 2.0 * n_gr * to_light,
            "reflectivities": g * lc * pw, "direction": g_refl - 2.0 * n_gr * n, "light_color": g * r * pw,
            "camera_position": g_to_cam, "shininess": g_k}


@lf._quiet
def specular_point(positions, normals, reflectivities, light_position, light_color, camera_position, shininess,
                   double_sided=True):
    shape, (p, n, r) = lf._rows(positions, normals, reflectivities)
    u = lf._over_length_eps(p - lf._f64(light_position))
    return _per_row_specular(p, n, r, u, light_color, camera_position, shininess, double_sided).reshape(shape)


@lf._quiet
def specular_point_vjp(positions, normals, reflectivities, light_position, light_color, camera_position, shininess,
                       double_sided, grad):
    """-> dict of d (sum out * grad) / d {positions, normals, reflectivities, light_position, light_color,
    camera_position, shininess}"""
    shape, (p, n, r, g) = lf._rows(positions, normals, reflectivities, grad)
    rel = p - lf._f64(light_position)
    t = _per_row_specular(p, n, r, lf._over_length_eps(rel), light_color, camera_position, shininess, double_sided, g)
    g_rel = lf._over_length_eps_vjp(rel, t["direction"])
    return {"positions": (t["positions"] + g_rel).reshape(shape), "normals": t["normals"].reshape(shape),
            "reflectivities": t["reflectivities"].reshape(shape), "light_position": -g_rel.sum(0),
            "light_color": t["light_color"].sum(0), "camera_position": t["camera_position"].sum(0),
            "shininess": t["shininess"].sum()}


# ---- one light on the rows of one frame

@lf._quiet
def _light_rows(p, n, c, g, vector, diffuse, specular, cam, k, two, point):
    """Every per-row term of one light: the parameter terms (vector, diffuse, specular [R,3]; camera [R,3];
    shininess [R,1]) and the adjoints (positions, normals, colors)."""
    vector, diffuse = lf._f64(vector), lf._f64(diffuse)
    if point:
        rel = p - vector
        l = lf._over_length_eps(rel)
        toward, sign = l, 1.0
    else:
        l = np.broadcast_to(vector, p.shape)
        toward, sign = -l, -1.0
    cos = lf._dot(n, toward)
    cs = lf._clamp(cos, two)
    g_cos = lf._clamp_vjp(cos, lf._dot(g, diffuse * c), two)
    s = _per_row_specular(p, n, c, l, specular, cam, k, two, g)
    g_l = sign * g_cos * n + s["direction"]
    pos = s["positions"]
    if point:
        g_rel = lf._over_length_eps_vjp(rel, g_l)
        pos, g_l = pos + g_rel, -g_rel
    return {"vectors": g_l, "diffuse": g * c * cs, "specular": s["light_color"], "camera": s["camera_position"],
            "shininess": s["shininess"], "positions": pos, "normals": g_cos * toward + s["normals"],
            "colors": g * diffuse * cs + s["reflectivities"]}


def _light_fwd_vjp(p, n, c, g, vector, diffuse, specular, cam, k, two, point):
    """(d, s, vjp or None) of one light from lighting_f64's functions and specular_point: the vjp as
    {vectors, diffuse, specular, camera, shininess, positions, normals, colors}"""
    if point:
        d = lf.diffuse_point(p, n, c, vector, diffuse, two)
        s = specular_point(p, n, c, vector, specular, cam, k, two)
    else:
        d = lf.diffuse_directional(n, c, vector, diffuse, two)
        s = lf.specular_directional(p, n, c, vector, specular, cam, k, two)
    if g is None:
        return d, s, None
    if point:
        dv = lf.diffuse_point_vjp(p, n, c, vector, diffuse, two, g)
        sv = specular_point_vjp(p, n, c, vector, specular, cam, k, two, g)
        vec, pos = dv["light_position"] + sv["light_position"], dv["positions"] + sv["positions"]
    else:
        dv = lf.diffuse_directional_vjp(n, c, vector, diffuse, two, g)
        sv = lf.specular_directional_vjp(p, n, c, vector, specular, cam, k, two, g)
        vec, pos = dv["light_direction"] + sv["light_direction"], sv["positions"]
    return d, s, {"vectors": vec, "diffuse": dv["light_color"], "specular": sv["light_color"],
                  "camera": sv["camera_position"], "shininess": sv["shininess"], "positions": pos,
                  "normals": dv["normals"] + sv["normals"], "colors": dv["colors"] + sv["reflectivities"]}


# ---- the parameters of one call

class LightSet:
    """float32 values, as both implementations receive them: vectors, diffuse, specular [N,3] or [B,N,3]; camera [3]
    or [B,3]; ambient [3] or None; shininess a number; point a tuple of N bools."""

    def __init__(self, vectors, diffuse, specular, camera, ambient, shininess, point, double_sided):
        self.vectors, self.diffuse, self.specular = (np.asarray(x, F32) for x in (vectors, diffuse, specular))
        self.camera = np.asarray(camera, F32)
        self.ambient = None if ambient is None else np.asarray(ambient, F32)
        self.shininess, self.point, self.double_sided = shininess, tuple(bool(b) for b in point), double_sided
        self.n = self.vectors.shape[-2]
        assert len(self.point) == self.n <= MAX_LIGHTS

    def frame(self, b):
        """(vectors [N,3], diffuse, specular, camera [3]) of frame b"""
        pick = lambda a, d: a[b] if a.ndim == d else a  # noqa: E731
        return pick(self.vectors, 3), pick(self.diffuse, 3), pick(self.specular, 3), pick(self.camera, 2)


KINDS = {"directional": lambda i: False, "point": lambda i: True, "mixed": lambda i: i % 2 == 1}


def draw_lights(rng, frames, n=2, kinds="mixed", per_frame=False, shininess=6.0, double_sided=False, ambient=True):
    """Lights from the generator `rng` for G-buffers whose positions lie in [-1, 1]^3 (shade_input's): directions of
    length 0.8 .. 1 (they are used raw; none longer than 1, so that no cosine is raised to the 50th power from above
    1), point positions 2.3 .. 3 from the origin -- at least 0.5 from every position -- colours in [0.1, 1];
    per_frame: one set and one camera (near deferred_cases.Lights().camera) per frame."""
    lead = (frames,) if per_frame else ()
    point = tuple(KINDS[kinds](i) for i in range(n))
    unit = rng.standard_normal(lead + (n, 3))
    unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
    radius = np.where(np.asarray(point, bool)[:, None], rng.uniform(2.3, 3.0, lead + (n, 1)),
                      rng.uniform(0.8, 1.0, lead + (n, 1)))
    vectors = (unit * radius).astype(F32)
    diffuse, specular = (rng.uniform(0.1, 1.0, lead + (n, 3)).astype(F32) for _ in range(2))
    camera = (np.asarray(dc.Lights().camera, np.float64) + (rng.uniform(-0.2, 0.2, lead + (3,)) if per_frame else 0.0))
    amb = rng.uniform(0.1, 1.0, 3).astype(F32) if ambient else None
    return LightSet(vectors, diffuse, specular, camera, amb, shininess, point, double_sided)


def light_set(ident, n=2, kinds="mixed", per_frame=False, shininess=6.0, double_sided=False, ambient=True):
    """draw_lights for the frame `ident` of the table, seeded by its name"""
    L = draw_lights(dc._rng(ident, 21, n, len(kinds), int(per_frame)), dict(FRAMES)[ident].shape[0], n, kinds,
                    per_frame, shininess, double_sided, ambient)
    positions = shade_input(ident)[0]
    finite = positions[np.isfinite(positions).all(-1)].astype(np.float64)
    for v in L.vectors.reshape((-1, n, 3) if n else (0, 0, 3)):
        for i in range(n):
            if L.point[i] and len(finite):
                assert np.linalg.norm(finite - v[i], axis=-1).min() >= 0.5
    return L


def random_input(rng, covered, invalid=None):
    """(positions, colors, normals) float32 over `covered` [B,H,W] bool, drawn as shade_input draws them: unit
    normals, positions in [-1, 1]^3, colours in [0.2, 1], -inf background; `invalid` [B,H,W] bool marks covered pixels
    whose normal is NaN (invalid without any dilation)."""
    shape = covered.shape + (3,)
    n = rng.standard_normal(shape)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    p = rng.uniform(-1.0, 1.0, shape).astype(F32)
    c = rng.uniform(0.2, 1.0, shape).astype(F32)
    p[~covered] = -np.inf
    n[~covered] = -np.inf
    if invalid is not None:
        n[invalid & covered] = np.nan
    return p, c, n


# ---- the statement

def shade_lights(positions, colors, normals, L, grad=None):
    """-> dict: pixels (float64), valid (bool [B,H,W]), route (uint32), scale (|ambient| + sum |d_i| + sum |s_i|, for
    the forward bound); with grad also the G-buffer gradients positions / colors / normals, `params` {name: gradient,
    shaped as the parameter (shininess: a number; ambient None: absent)} and `absum` {name: the sum of the absolute
    per-pixel terms, same shapes}.  [H,W,3] inputs give unbatched results."""
    squeeze, rp, rn, valid, P, N, C = dc._shade_terms(positions, colors, normals, None)
    B, H, W = valid.shape
    pixels, scale = np.zeros(P.shape), np.zeros(P.shape)
    out = {"valid": valid,
           "route": (rp | (rn << np.uint32(12)) | (valid.astype(np.uint32) << np.uint32(31))).astype(np.uint32)}
    amb = np.zeros(3) if L.ambient is None else np.asarray(L.ambient, np.float64)
    if grad is not None:
        G = np.asarray(dc._batched(grad)[0], np.float64)
        a_pos, a_nrm, a_col = np.zeros(P.shape), np.zeros(P.shape), np.zeros(P.shape)
        shapes = {"vectors": L.vectors.shape, "diffuse": L.diffuse.shape, "specular": L.specular.shape,
                  "camera": L.camera.shape, "ambient": (3,), "shininess": ()}
        params = {k: np.zeros(s) for k, s in shapes.items()}
        absum = {k: np.zeros(s) for k, s in shapes.items()}
    for b in range(B):
        sel = valid[b]
        p, n, c = P[b][sel], N[b][sel], C[b][sel]
        g = None if grad is None else G[b][sel]
        vectors, diffuse, specular, cam = L.frame(b)
        acc, sc = np.zeros(p.shape), np.abs(c * amb)
        for i in range(L.n):
            d, s, vjp = _light_fwd_vjp(p, n, c, g, vectors[i], diffuse[i], specular[i], cam, L.shininess,
                                       L.double_sided, L.point[i])
            acc = (d + s) if i == 0 else acc + (d + s)
            sc = sc + np.abs(d) + np.abs(s)
            if g is None:
                continue
            a_pos[b][sel] += vjp["positions"]
            a_nrm[b][sel] += vjp["normals"]
            a_col[b][sel] += vjp["colors"]
            rows = _light_rows(p, n, c, g, vectors[i], diffuse[i], specular[i], cam, L.shininess, L.double_sided,
                               L.point[i])
            for name in ("vectors", "diffuse", "specular", "camera", "shininess"):
                at = ((b,) if params[name].ndim == (3 if name != "camera" else 2) else ())
                if name in ("vectors", "diffuse", "specular"):
                    at = at + (i,)
                params[name][at] += vjp[name]
                absum[name][at] += np.abs(rows[name]).sum(0).reshape(np.shape(vjp[name]))
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
        out["colors"] = a_col
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


def param_ratio(got, ref, absum, frac):
    """worst |got - ref| / (frac * absum) over a parameter's elements (0 / 0 counts as 0; a NaN as a failure)"""
    got, ref, absum = (np.asarray(x, np.float64).reshape(-1) for x in (got, ref, absum))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / (frac * absum))
    return float(np.inf if np.isnan(ratio).any() else ratio.max(initial=0.0))


# ---- references, computed once per process and shared by the tests (treat as read-only)

@functools.lru_cache(maxsize=None)
def case(ident, n=2, kinds="mixed", per_frame=False, shininess=6.0, double_sided=False, ambient=True):
    """(inputs, LightSet, upstream gradient float32, statement dict with gradients) for one frame of the table"""
    inputs = shade_input(ident)
    L = light_set(ident, n, kinds, per_frame, shininess, double_sided, ambient)
    grad = dc._rng(ident, 9).standard_normal(inputs[0].shape).astype(F32)
    return inputs, L, grad, shade_lights(*inputs, L, grad)


def accuracy_frames():
    """the frames whose parameter gradients are held to GRAD_FRAC * absum: all but the 1x1 ones (a single pixel's
    specular cosine cancels there; measured with the framework ops in float32 at 7.1 of the bound)"""
    return [i for i in dc.FRAME_IDS if not i.startswith("1x1-")]
