"""Float64 numpy statement of the reference's lighting helpers, forward and backward.  TEST INFRASTRUCTURE ONLY.

An independent statement next to dirt_amd/lighting.py (`_*_ops`, framework ops differentiated by autograd) and
dirt_amd/csrc/lighting_kernels.h (fused float32 HIP kernels): written from the reference's formulas
(dirt/lighting.py: face normals :24-31, vertex_normals :34-93, diffuse_directional :219-225,
specular_directional :276-288, diffuse_point :335-343) in numpy float64, with hand-derived vector-Jacobian
products -- no torch, no autograd, and no code shared with either.

Formulas (eps = 1e-12, a float64 here and a float32 in the kernels: where a length is exactly 0 the two differ
by 4e-9 relative, so such rows are compared relatively):
  * face normal   nf = (v1 - v0) x (v2 - v0),  nf / (|nf| + eps); summed into the face's three vertices;
    vertex normal  s / (|s| + eps).  Only x, y, z of a [.., V, 4] vertex are read; w gets a zero gradient.
  * diffuse_directional   cos = n . (-l);                          out = light_color * colour * clamp(cos)
  * specular_directional  r = l + 2 (n . (-l)) n,  t = cam - p,  cos = (t / |t| + eps) . r  (eps is added to the
    unit VECTOR, dirt/lighting.py:280);                         out = light_color * refl * clamp(cos) ** k
  * diffuse_point         d = p - light,  cos = n . d / (|d| + eps); out = light_color * colour * clamp(cos)
  clamp(x) = |x| (double_sided) or max(x, 0).

Conventions at the kinks -- what the framework ops do (checked with torch on a CPU), and TensorFlow's Maximum
rule x >= y as well:
  * d|x| = sign(x), 0 at x = 0;
  * max(x, 0) passes the gradient where x >= 0;
  * d|v| at v = 0 is 0 (the vector length's subgradient);
  * d x^k = k x^(k-1), identically 0 for k = 0; the clamp's gradient is applied after it as a SELECT, so a
    back-facing one-sided point gets exactly 0 and never 0 * inf (k < 1);
  * NaN propagates through both clamps in the forward (|NaN| = NaN, max(NaN, 0) = NaN);
  * the gradient through a clamp whose argument is NaN is 0.
Faces with an index outside [0, V) contribute nothing, forward or backward (the fused path's documented rule;
the framework's index_select rejects them).
"""
import numpy as np

EPS = 1.e-12
_quiet = np.errstate(all="ignore")  # non-finite operands are part of the contract: they propagate silently


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _length(x):
    return np.sqrt(np.square(x).sum(-1, keepdims=True))


def _dot(a, b):
    return (a * b).sum(-1, keepdims=True)


def _over_length_eps(x):
    """x / (|x| + eps)"""
    return x / (_length(x) + EPS)


def _over_length_eps_vjp(x, g):
    """J^T g of x -> x / (|x| + eps): with h the unit vector of x (0 at x = 0, the length's subgradient) and
    d = |x| + eps, the Jacobian is I / d - h h^T |x| / d^2 (symmetric)."""
    m = _length(x)
    d = m + EPS
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(m > 0, x / np.where(m > 0, m, 1.0), 0.0)
        return g / d - h * _dot(h, g) * (m / (d * d))


def _clamp(c, double_sided):
    return np.abs(c) if double_sided else np.maximum(c, 0.0)  # (np.maximum propagates NaN)


def _clamp_vjp(c, g, double_sided):
    """A select on the clamp's argument, never a product: 0 where the argument is NaN."""
    if double_sided:
        return np.where(c > 0, g, np.where(c < 0, -g, 0.0))
    return np.where(c >= 0, g, 0.0)


def _skew(a):
    """[a]x with [a]x b = a x b; a [..., 3] -> [..., 3, 3]"""
    z = np.zeros_like(a[..., 0])
    return np.stack([np.stack([z, -a[..., 2], a[..., 1]], -1),
                     np.stack([a[..., 2], z, -a[..., 0]], -1),
                     np.stack([-a[..., 1], a[..., 0], z], -1)], -2)


# ---- vertex_normals

def _valid_faces(faces, V):
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    return faces[np.all((faces >= 0) & (faces < V), axis=1)]


def _vn_terms(vertices, faces):
    v = _f64(vertices)
    shape = v.shape
    xyz = v.reshape((int(np.prod(shape[:-2])),) + shape[-2:])[..., :3]  # [B, V, 3]
    faces = _valid_faces(faces, shape[-2])
    corners = xyz[:, faces]  # [B, F, 3 (corner), 3]
    e1, e2 = corners[:, :, 1] - corners[:, :, 0], corners[:, :, 2] - corners[:, :, 0]
    nf = np.einsum("...ij,...j->...i", _skew(e1), e2)
    summed = np.zeros_like(xyz)
    unit = _over_length_eps(nf)
    for k in range(3):
        np.add.at(summed, (slice(None), faces[:, k]), unit)
    return shape, xyz, faces, e1, e2, nf, summed


@_quiet
def vertex_normals(vertices, faces):
    """vertices [*, V, D >= 3], faces [F, 3] (any integer type) -> normals [*, V, 3]"""
    shape, _, _, _, _, _, summed = _vn_terms(vertices, faces)
    return _over_length_eps(summed).reshape(shape[:-1] + (3,))


@_quiet
def vertex_normals_vjp(vertices, faces, grad):
    """d (sum normals * grad) / d vertices, in vertices' shape (w, if present, gets 0)."""
    shape, xyz, faces, e1, e2, nf, summed = _vn_terms(vertices, faces)
    g_summed = _over_length_eps_vjp(summed, _f64(grad).reshape(summed.shape))
    # every face's unit normal went to its three corners: it receives the sum of theirs
    g_unit = g_summed[:, faces[:, 0]] + g_summed[:, faces[:, 1]] + g_summed[:, faces[:, 2]]  # [B, F, 3]
    g_nf = _over_length_eps_vjp(nf, g_unit)
    # nf = [e1]x e2 = -[e2]x e1:  J_e2 = [e1]x,  J_e1 = -[e2]x;  J^T g with [a]x^T = -[a]x
    g_e1 = np.einsum("...ji,...j->...i", -_skew(e2), g_nf)
    g_e2 = np.einsum("...ji,...j->...i", _skew(e1), g_nf)
    out = np.zeros(xyz.shape[:2] + (shape[-1],))
    np.add.at(out[..., :3], (slice(None), faces[:, 1]), g_e1)
    np.add.at(out[..., :3], (slice(None), faces[:, 2]), g_e2)
    np.add.at(out[..., :3], (slice(None), faces[:, 0]), -(g_e1 + g_e2))
    return out.reshape(shape)


# ---- elementwise helpers: operands [..., 3] of one shape, light parameters [3]

def _rows(*xs):
    xs = [_f64(x) for x in xs]
    return xs[0].shape, [x.reshape(-1, 3) for x in xs]


@_quiet
def diffuse_directional(normals, colors, light_direction, light_color, double_sided=True):
    shape, (n, c) = _rows(normals, colors)
    cos = _dot(n, -_f64(light_direction))
    return (_f64(light_color) * c * _clamp(cos, double_sided)).reshape(shape)


@_quiet
def diffuse_directional_vjp(normals, colors, light_direction, light_color, double_sided, grad):
    """-> dict of d (sum out * grad) / d {normals, colors, light_direction, light_color}"""
    shape, (n, c, g) = _rows(normals, colors, grad)
    ld, lc = _f64(light_direction), _f64(light_color)
    cos = _dot(n, -ld)
    cs = _clamp(cos, double_sided)
    g_cos = _clamp_vjp(cos, _dot(g, lc * c), double_sided)
    return {"normals": (g_cos * -ld).reshape(shape), "colors": (g * lc * cs).reshape(shape),
            "light_direction": -(g_cos * n).sum(0), "light_color": (g * c * cs).sum(0)}


def _power(cs, k):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.power(cs, float(k))


def _power_slope(cs, k):
    if float(k) == 0.0:
        return np.zeros_like(cs)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(k) * np.power(cs, float(k) - 1.0)


def _spec_terms(p, n, ld, cam):
    to_light = -ld
    reflected = ld + 2.0 * _dot(n, to_light) * n
    to_cam = cam - p
    with np.errstate(invalid="ignore", divide="ignore"):
        view = to_cam / _length(to_cam) + EPS
    return to_light, reflected, to_cam, view


@_quiet
def specular_directional(positions, normals, reflectivities, light_direction, light_color, camera_position,
                         shininess, double_sided=True):
    shape, (p, n, r) = _rows(positions, normals, reflectivities)
    _, reflected, _, view = _spec_terms(p, n, _f64(light_direction), _f64(camera_position))
    cs = _clamp(_dot(view, reflected), double_sided)
    return (_f64(light_color) * r * _power(cs, shininess)).reshape(shape)


@_quiet
def specular_directional_vjp(positions, normals, reflectivities, light_direction, light_color, camera_position,
                             shininess, double_sided, grad):
    """-> dict of d (sum out * grad) / d {positions, normals, reflectivities, light_direction, light_color,
    camera_position, shininess}"""
    shape, (p, n, r, g) = _rows(positions, normals, reflectivities, grad)
    ld, lc, cam = _f64(light_direction), _f64(light_color), _f64(camera_position)
    to_light, reflected, to_cam, view = _spec_terms(p, n, ld, cam)
    cos = _dot(view, reflected)
    cs = _clamp(cos, double_sided)
    pw = _power(cs, shininess)
    g_pw = _dot(g, lc * r)
    with np.errstate(invalid="ignore", divide="ignore"):
        g_cos = _clamp_vjp(cos, g_pw * _power_slope(cs, shininess), double_sided)
        g_view, g_refl = g_cos * reflected, g_cos * view
        # view = to_cam / |to_cam| + eps: the projection off the unit vector, over the length
        tl = _length(to_cam)
        h = to_cam / tl
        g_to_cam = (g_view - h * _dot(h, g_view)) / tl
        # d cs^k / dk = cs^k ln cs, 0 at cs = 0 (the framework's rule for a zero base)
        g_k = (g_pw * np.where(cs > 0, pw * np.log(np.where(cs > 0, cs, 1.0)), np.where(cs == 0, 0.0, np.nan))).sum()
    # reflected = ld + 2 s n with s = n . to_light = -(n . ld)
    s, n_gr = _dot(n, to_light), _dot(n, g_refl)
    return {"positions": (-g_to_cam).reshape(shape),
            "normals": (2.0 * s * g_refl + 2.0 * n_gr * to_light).reshape(shape),
            "reflectivities": (g * lc * pw).reshape(shape), "light_direction": (g_refl - 2.0 * n_gr * n).sum(0),
            "light_color": (g * r * pw).sum(0), "camera_position": g_to_cam.sum(0), "shininess": g_k}


@_quiet
def diffuse_point(positions, normals, colors, light_position, light_color, double_sided=True):
    shape, (p, n, c) = _rows(positions, normals, colors)
    incident = _over_length_eps(p - _f64(light_position))
    return (_f64(light_color) * c * _clamp(_dot(n, incident), double_sided)).reshape(shape)


@_quiet
def diffuse_point_vjp(positions, normals, colors, light_position, light_color, double_sided, grad):
    """-> dict of d (sum out * grad) / d {positions, normals, colors, light_position, light_color}"""
    shape, (p, n, c, g) = _rows(positions, normals, colors, grad)
    lc = _f64(light_color)
    rel = p - _f64(light_position)
    incident = _over_length_eps(rel)
    cos = _dot(n, incident)
    cs = _clamp(cos, double_sided)
    g_cos = _clamp_vjp(cos, _dot(g, lc * c), double_sided)
    g_rel = _over_length_eps_vjp(rel, g_cos * n)
    return {"positions": g_rel.reshape(shape), "normals": (g_cos * incident).reshape(shape),
            "colors": (g * lc * cs).reshape(shape), "light_position": -g_rel.sum(0),
            "light_color": (g * c * cs).sum(0)}
