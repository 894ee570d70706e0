"""Statement of record for deferred.reflect_view and deferred.shade_env (dirt_amd/deferred.py,
dirt_amd/csrc/shade_env_kernels.h): numpy float64, no torch and no code shared with either implementation.  TEST
INFRASTRUCTURE ONLY.

Dilation of positions and normals under the positions' background, `valid` and the route word are
tests/deferred_cases.py's; colours, material, radiance and occlusion are read at the pixel itself.  For a valid pixel
with dilated position p, dilated normal n_d, colour c, material (r_0, m_0), u(x) = x / (|x| + 1e-12), in this order:

reflect_view
    n = u(n_d)   v = u(cam - p)   nvr = n . v (not clamped)   t = 2 nvr   R = t n - v
and exactly (0, 0, 0) at an invalid pixel.

shade_env
    n = u(n_d)   v = u(cam - p)   nv = max(n . v, 0)
    r = clamp(r_0, R_MIN, 1)   m = clamp(m_0, 0, 1)
    E = coeff_0 Y_0;  E = E + coeff_k Y_k(n)      (tests/shade_sh_cases.basis, in index order)
    F0 = 0.04 + (c - 0.04) m
    x = 1 - r   y = 0.0425 - 0.0275 r   z = 1.04 - 0.572 r   w = 0.022 r - 0.04
    e = exp2(-9.28 nv)   q = x x   s = q < e ? q : e   a = s x + y   A = z - 1.04 a   B = 1.04 a + w
    S = F0 A + B   dif = ((1 - m) c) E   spec = radiance S   pixels = occlusion (dif + spec)
and exactly 0 at an invalid pixel.  Every clamp takes torch.clamp's derivative (the gradient passes where
min <= x <= max, ends included), max(., 0) passes it where its argument is >= 0, the select passes it to the chosen
side only, u's subgradient at 0 is 0 (lighting_f64's rule).

Gradients, derived by hand in `reflect_rows` and `env_rows` (checked against central differences by
tests/test_shade_env_cpu.py): the adjoints of the dilated position and normal are routed through the dilation by
deferred_cases.gather; colours, material, radiance and occlusion receive their own pixel's terms; a parameter's
gradient is the sum of its per-pixel terms over the valid pixels of its frame (per-frame parameters) or of all frames
(shared ones).  `absum` is, per parameter element, the sum over those pixels of the absolute per-pixel terms: the scale
a float32 sum of those terms is judged by.  `scale` = |occlusion| (|dif| + |spec|) for shade_env, 1 for reflect_view (a
unit-length output).

The forward bound is k FWD_ATOL + FWD_RTOL scale with k the number of terms a pixel's value is added up from: 2 for
reflect_view (t n and v), K + 2 for shade_env (the K terms of E, and F0 A and B of S).
"""
import functools

import numpy as np

import deferred_cases as dc
import lighting_cases
import lighting_f64 as lf
import shade_sh_cases as ssc
from deferred_cases import FRAMES, FRAME_IDS  # noqa: F401  (the frame table, reused)
from shade_sh_cases import param_ratio  # noqa: F401  (the parameter comparison, reused)

F32 = np.float32
COUNTS = ssc.COUNTS
R_MIN = float(F32(0.045))
MARGIN = 1e-3  # every generated pixel is at least this far from each kink
PIXEL_NAMES = ("positions", "colors", "normals", "material", "radiance", "occlusion")
PARAMS = ("coefficients", "camera")
LN2 = float(np.log(2.0))


def _clamp_pass(x, lo, hi):
    """torch.clamp's derivative: 1 where lo <= x <= hi"""
    return ((x >= lo) & (x <= hi)).astype(np.float64)


def _view(p, nd, cam):
    n = lf._over_length_eps(nd)
    tc = lf._f64(cam) - p
    v = lf._over_length_eps(tc)
    return n, tc, v, lf._dot(n, v)


@lf._quiet
def reflect_rows(p, nd, g, cam):
    """rows p, nd [R,3], g [R,3] or None, cam [3] -> dict: directions; with g the per-row adjoints positions, normals
    (of the dilated values) and the per-row camera terms"""
    n, tc, v, nvr = _view(p, nd, cam)
    t = 2.0 * nvr
    out = {"directions": t * n - v}
    if g is None:
        return out
    g_nvr = 2.0 * lf._dot(g, n)
    g_n = t * g + g_nvr * v
    g_v = g_nvr * n - g
    g_tc = lf._over_length_eps_vjp(tc, g_v)
    out.update({"positions": -g_tc, "normals": lf._over_length_eps_vjp(nd, g_n), "camera": g_tc})
    return out


@lf._quiet
def env_rows(p, nd, c, mat, rad, occ, g, coef, cam):
    """rows p, nd, c, rad [R,3], mat [R,2], occ [R,1], g [R,3] or None, coef [K,3], cam [3] (float64) -> dict: pixels,
    scale, and the distances nvr, qe (= q - e) to the two kinks of the geometry; with g every per-row adjoint:
    positions, normals (of the dilated values), colors, material [R,2], radiance, occlusion [R,1], and the per-row
    parameter terms camera [R,3], coefficients [R,K,3]"""
    coef = lf._f64(coef)
    K = coef.shape[0]
    n, tc, v, nvr = _view(p, nd, cam)
    nv = np.maximum(nvr, 0.0)
    r0, m0 = mat[:, 0:1], mat[:, 1:2]
    r = np.minimum(np.maximum(r0, R_MIN), 1.0)
    m = np.minimum(np.maximum(m0, 0.0), 1.0)
    Y, _, dY = ssc.basis(n, K)
    E = coef[0] * Y[:, 0:1]
    for k in range(1, K):
        E = E + coef[k] * Y[:, k:k + 1]
    F0 = 0.04 + (c - 0.04) * m
    x = 1.0 - r
    y = 0.0425 - 0.0275 * r
    z = 1.04 - 0.572 * r
    w = 0.022 * r - 0.04
    e = np.exp2(-9.28 * nv)
    q = x * x
    on_q = q < e
    s = np.where(on_q, q, e)
    a = s * x + y
    A = z - 1.04 * a
    Bq = 1.04 * a + w
    S = F0 * A + Bq
    kd = (1.0 - m) * c
    dif = kd * E
    spec = rad * S
    out = {"pixels": occ * (dif + spec), "scale": np.abs(occ) * (np.abs(dif) + np.abs(spec)), "nvr": nvr, "qe": q - e}
    if g is None:
        return out
    g_occ = lf._dot(g, dif + spec)
    gt = g * occ
    g_kd = gt * E
    gE = gt * kd
    g_rad = gt * S
    gS = gt * rad
    g_F0 = gS * A
    g_A = lf._dot(gS, F0)
    g_B = gS.sum(-1, keepdims=True)
    g_c = g_kd * (1.0 - m) + g_F0 * m
    g_m = -lf._dot(g_kd, c) + lf._dot(g_F0, c - 0.04)
    g_a = 1.04 * (g_B - g_A)
    g_s = g_a * x
    g_x = g_a * s + np.where(on_q, 2.0 * x * g_s, 0.0)
    g_e = np.where(on_q, 0.0, g_s)
    g_nv = g_e * e * (LN2 * -9.28)
    g_r = -g_x - 0.0275 * g_a - 0.572 * g_A + 0.022 * g_B
    g_nvr = g_nv * (nvr >= 0)
    terms = Y[:, :, None] * gE[:, None, :]  # [R,K,3]
    wk = gE @ coef.T  # [R,K]: sum_c gE_c coefficients[k,c]
    g_n = (wk[:, :, None] * dY).sum(1) + g_nvr * v
    g_v = g_nvr * n
    g_tc = lf._over_length_eps_vjp(tc, g_v)
    out.update({"positions": -g_tc, "normals": lf._over_length_eps_vjp(nd, g_n), "colors": g_c,
                "material": np.concatenate([g_r * _clamp_pass(r0, R_MIN, 1.0), g_m * _clamp_pass(m0, 0.0, 1.0)], -1),
                "radiance": g_rad, "occlusion": g_occ, "camera": g_tc, "coefficients": terms})
    return out


# ---- the parameters of one call

class Env:
    """float32 values, as both implementations receive them: coefficients [K,3] or [B,K,3]; camera [3] or [B,3]."""

    def __init__(self, coefficients, camera):
        self.coefficients, self.camera = np.asarray(coefficients, F32), np.asarray(camera, F32)
        self.K = self.coefficients.shape[-2]
        assert self.K in COUNTS

    def frame(self, b):
        """(coefficients [K,3], camera [3]) of frame b"""
        return (self.coefficients[b] if self.coefficients.ndim == 3 else self.coefficients,
                self.camera[b] if self.camera.ndim == 2 else self.camera)

    def pick(self, frames):
        """the parameters of the frames `frames` alone"""
        return Env(self.coefficients[frames] if self.coefficients.ndim == 3 else self.coefficients,
                   self.camera[frames] if self.camera.ndim == 2 else self.camera)


def draw_env(rng, frames, K=9, per_frame=False):
    """coefficients in [-1, 1] (the constant term in [0.5, 1.5]); the camera near deferred_cases.Lights().camera, one
    per frame with per_frame"""
    lead = (frames,) if per_frame else ()
    coef = rng.uniform(-1.0, 1.0, lead + (K, 3))
    coef[..., 0, :] = rng.uniform(0.5, 1.5, lead + (3,))
    camera = np.asarray(dc.Lights().camera, np.float64) + (rng.uniform(-0.2, 0.2, lead + (3,)) if per_frame else 0.0)
    return Env(coef, camera)


# ---- the statements

def reflect_view(positions, normals, camera, grad=None):
    """-> dict: directions (float64), valid (bool [B,H,W]), route (uint32), scale (ones); with grad also positions,
    normals, `params` {"camera"} and `absum`.  camera [3] or [B,3].  [H,W,3] inputs give unbatched results."""
    squeeze, rp, rn, valid, P, N, _ = dc._shade_terms(positions, positions, normals, None)
    B = valid.shape[0]
    camera = np.asarray(camera)  # (float32 as the implementations receive it; any dtype is taken as it is)
    out = {"valid": valid, "scale": np.ones(P.shape),
           "route": (rp | (rn << np.uint32(12)) | (valid.astype(np.uint32) << np.uint32(31))).astype(np.uint32)}
    directions = np.zeros(P.shape)
    if grad is not None:
        G = np.asarray(dc._batched(grad)[0], np.float64)
        a_pos, a_nrm = np.zeros(P.shape), np.zeros(P.shape)
        params, absum = {"camera": np.zeros(camera.shape)}, {"camera": np.zeros(camera.shape)}
    for b in range(B):
        sel = valid[b]
        t = reflect_rows(P[b][sel], N[b][sel], None if grad is None else G[b][sel],
                         camera[b] if camera.ndim == 2 else camera)
        directions[b][sel] = t["directions"]
        if grad is None:
            continue
        a_pos[b][sel], a_nrm[b][sel] = t["positions"], t["normals"]
        at = (b,) if camera.ndim == 2 else ()
        params["camera"][at] += t["camera"].sum(0)
        absum["camera"][at] += np.abs(t["camera"]).sum(0)
    out["directions"] = directions
    if grad is not None:
        out["positions"] = dc.gather(a_pos, dc.codes(rp, 3))[0]
        out["normals"] = dc.gather(a_nrm, dc.codes(rn, 3))[0]
        out["params"], out["absum"] = params, absum
    if squeeze:
        out = {k: (a if k in ("params", "absum") else a[0]) for k, a in out.items()}
    return out


def shade_env(positions, colors, normals, material, radiance, occlusion, L, grad=None):
    """-> dict: pixels (float64), valid (bool [B,H,W]), route (uint32), scale (for the forward bound), nvr and qe (the
    distances to the geometry's kinks, inf at an invalid pixel); with grad also the per-pixel gradients positions /
    colors / normals / material / radiance / occlusion, `params` {"coefficients", "camera"} (shaped as the parameters)
    and `absum` (same shapes).  occlusion None is ones.  [H,W,.] inputs give unbatched results."""
    squeeze, rp, rn, valid, P, N, C = dc._shade_terms(positions, colors, normals, None)
    B, H, W = valid.shape
    M = np.asarray(dc._batched(material)[0], np.float64)
    R = np.asarray(dc._batched(radiance)[0], np.float64)
    O = np.ones((B, H, W, 1)) if occlusion is None else np.asarray(dc._batched(occlusion)[0], np.float64)
    pixels, scale = np.zeros(P.shape), np.zeros(P.shape)
    nvr, qe = np.full((B, H, W), np.inf), np.full((B, H, W), np.inf)
    out = {"valid": valid,
           "route": (rp | (rn << np.uint32(12)) | (valid.astype(np.uint32) << np.uint32(31))).astype(np.uint32)}
    if grad is not None:
        G = np.asarray(dc._batched(grad)[0], np.float64)
        adj = {"positions": np.zeros(P.shape), "normals": np.zeros(P.shape), "colors": np.zeros(P.shape),
               "material": np.zeros(M.shape), "radiance": np.zeros(R.shape), "occlusion": np.zeros(O.shape)}
        shapes = {"coefficients": L.coefficients.shape, "camera": L.camera.shape}
        params = {k: np.zeros(s) for k, s in shapes.items()}
        absum = {k: np.zeros(s) for k, s in shapes.items()}
    for b in range(B):
        sel = valid[b]
        coef, cam = L.frame(b)
        t = env_rows(P[b][sel], N[b][sel], C[b][sel], M[b][sel], R[b][sel], O[b][sel],
                     None if grad is None else G[b][sel], coef, cam)
        pixels[b][sel], scale[b][sel] = t["pixels"], t["scale"]
        nvr[b][sel], qe[b][sel] = t["nvr"][:, 0], t["qe"][:, 0]
        if grad is None:
            continue
        for name in adj:
            adj[name][b][sel] = t[name]
        for name, dim in (("coefficients", 3), ("camera", 2)):
            at = (b,) if params[name].ndim == dim else ()
            params[name][at] += t[name].sum(0)
            absum[name][at] += np.abs(t[name]).sum(0)
    out.update({"pixels": pixels, "scale": scale, "nvr": nvr, "qe": qe})
    if grad is not None:
        out["positions"] = dc.gather(adj["positions"], dc.codes(rp, 3))[0]
        out["normals"] = dc.gather(adj["normals"], dc.codes(rn, 3))[0]
        for name in ("colors", "material", "radiance", "occlusion"):
            out[name] = adj[name]
        out["params"], out["absum"] = params, absum
    if squeeze:
        out = {k: (a if k in ("params", "absum") else a[0]) for k, a in out.items()}
    return out


def reflect_fwd_bound(ref):
    """The lighting contract (tests/lighting_cases.py): two terms, a unit-length output"""
    return 2 * lighting_cases.FWD_ATOL + lighting_cases.FWD_RTOL * ref["scale"]


def fwd_bound(ref, K):
    """The lighting contract per term and summed: the K terms of E, and F0 A and B"""
    return (K + 2) * lighting_cases.FWD_ATOL + lighting_cases.FWD_RTOL * ref["scale"]


# ---- inputs: every valid pixel at least MARGIN away from each kink

def _away(x, ends):
    """x with the values closer than 2 MARGIN to one of `ends` moved to 2 MARGIN past it on their own side"""
    x = x.copy()
    for end in ends:
        near = np.abs(x - end) < 2 * MARGIN
        x[near] = np.where(x[near] < end, end - 2 * MARGIN, end + 2 * MARGIN)
    return x


def kink_distance(inputs, L):
    """the least distance of a valid pixel to a kink: n . v = 0, q = e, and the clamps' ends of the material"""
    ref = shade_env(*inputs, L)
    v = ref["valid"]
    mat = np.asarray(dc._batched(inputs[3])[0], np.float64)[v]
    ends = min(np.abs(mat[:, 0] - R_MIN).min(initial=np.inf), np.abs(mat[:, 0] - 1.0).min(initial=np.inf),
               np.abs(mat[:, 1]).min(initial=np.inf), np.abs(mat[:, 1] - 1.0).min(initial=np.inf))
    return min(float(np.abs(ref["nvr"]).min(initial=np.inf)), float(np.abs(ref["qe"]).min(initial=np.inf)), float(ends))


def settle(rng, inputs, L, pinned_material=False):
    """`inputs` with every valid pixel at least MARGIN from the kinks: the material moved off the clamps' ends and, at
    a pixel on q = e, redrawn (unless pinned_material); the finite normals in the 3x3 window of a pixel on n . v = 0
    (with pinned_material also q = e) redrawn.  The background and the NaN normals stay where they are."""
    p, c, n, mat, rad, occ = inputs
    n, mat = n.copy(), mat.copy()
    if not pinned_material:
        mat[..., 0] = _away(mat[..., 0], (R_MIN, 1.0))
        mat[..., 1] = _away(mat[..., 1], (0.0, 1.0))
    B, H, W = n.shape[:3]
    for _ in range(100):
        ref = shade_env(p, c, n, mat, rad, occ, L)
        on_nv, on_qe = np.abs(ref["nvr"]) < 2 * MARGIN, np.abs(ref["qe"]) < 2 * MARGIN
        if not on_nv.any() and not on_qe.any():
            break
        if not pinned_material:
            mat[..., 0][on_qe] = rng.uniform(0.1, 0.9, int(on_qe.sum())).astype(F32)
        for b, y, x in np.argwhere(on_nv | (on_qe if pinned_material else False)):
            ys, xs = slice(max(y - 1, 0), y + 2), slice(max(x - 1, 0), x + 2)
            window = n[b, ys, xs]
            finite = np.isfinite(window).all(-1)
            fresh = rng.standard_normal(window.shape)
            fresh = (fresh / np.linalg.norm(fresh, axis=-1, keepdims=True)).astype(F32)
            window[finite] = fresh[finite]
    out = (p, c, n, mat, rad, occ)
    assert kink_distance(out, L) >= MARGIN or pinned_material
    return out


def random_input(rng, covered, invalid=None, roughness=(0.0, 1.2), metallic=(-0.2, 1.2)):
    """(positions, colors, normals, material, radiance, occlusion) float32 over `covered` [B,H,W] bool: unit normals,
    positions in [-1, 1]^3, colours in [0.2, 1], -inf background in positions and normals; roughness and metallic in
    the given ranges (past the clamps' ends on purpose), radiance in [0, 2] and occlusion [B,H,W,1] in [0.2, 1]
    everywhere; `invalid` marks covered pixels whose normal is NaN.  Not yet settled."""
    shape = covered.shape + (3,)
    n = rng.standard_normal(shape)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    p = rng.uniform(-1.0, 1.0, shape).astype(F32)
    c = rng.uniform(0.2, 1.0, shape).astype(F32)
    mat = np.stack([rng.uniform(*roughness, covered.shape), rng.uniform(*metallic, covered.shape)], -1).astype(F32)
    rad = rng.uniform(0.0, 2.0, shape).astype(F32)
    occ = rng.uniform(0.2, 1.0, covered.shape + (1,)).astype(F32)
    p[~covered] = -np.inf
    n[~covered] = -np.inf
    if invalid is not None:
        n[invalid & covered] = np.nan
    return p, c, n, mat, rad, occ


def settled_input(rng, covered, L, invalid=None):
    return settle(rng, random_input(rng, covered, invalid), L)


# ---- references, computed once per process and shared by the tests (treat as read-only)

def env_of(ident, K=9, per_frame=False):
    return draw_env(dc._rng(ident, 41, K, int(per_frame)), dict(FRAMES)[ident].shape[0], K, per_frame)


@functools.lru_cache(maxsize=None)
def frame_input(ident, K=9, per_frame=False):
    """deferred_cases.shade_input's positions and colours with normals, a material, a radiance and an occlusion drawn
    and settled for them under env_of's camera"""
    p, c, _ = dc.shade_input(ident)
    rng = dc._rng(ident, 42, K, int(per_frame))
    drawn = random_input(rng, dict(FRAMES)[ident])
    return settle(rng, (p, c) + drawn[2:], env_of(ident, K, per_frame))


@functools.lru_cache(maxsize=None)
def case(ident, K=9, per_frame=False, occlusion=True):
    """(inputs (positions, colors, normals, material, radiance, occlusion or None), Env, upstream gradient float32,
    statement dict with gradients) for one frame of the table"""
    inputs = frame_input(ident, K, per_frame)
    if not occlusion:
        inputs = inputs[:5] + (None,)
    L = env_of(ident, K, per_frame)
    grad = dc._rng(ident, 9).standard_normal(inputs[0].shape).astype(F32)
    return inputs, L, grad, shade_env(*inputs, L, grad)


@functools.lru_cache(maxsize=None)
def reflect_case(ident, per_frame=False):
    """(positions, normals, camera float32, upstream gradient float32, statement dict with gradients) for one frame of
    the table: `case`'s positions, normals and camera"""
    p, _, n = frame_input(ident, 9, per_frame)[:3]
    camera = env_of(ident, 9, per_frame).camera
    grad = dc._rng(ident, 10).standard_normal(p.shape).astype(F32)
    return p, n, camera, grad, reflect_view(p, n, camera, grad)


@functools.lru_cache(maxsize=None)
def clamp_ends_case():
    """15x17-hole with the material exactly on the clamps' ends and past them, all exactly representable: roughness
    in {0, float32(0.045), 1, 1.5}, metallic in {-0.5, 0, 1, 1.5}, every combination present.  The closed-interval
    derivative passes at 0.045, 1 (roughness) and 0, 1 (metallic); a roughness of 0 and the values past the ends get
    exactly 0.  The geometry stays MARGIN away from its own kinks."""
    ident = "15x17-hole"
    L = env_of(ident)
    p, c, n, mat, rad, occ = frame_input(ident)
    rough = np.array([0.0, F32(0.045), 1.0, 1.5], F32)
    metal = np.array([-0.5, 0.0, 1.0, 1.5], F32)
    i = np.arange(mat[..., 0].size).reshape(mat.shape[:-1])
    mat = np.stack([rough[i % 4], metal[(i // 4) % 4]], -1)
    inputs = settle(dc._rng(ident, 43), (p, c, n, mat, rad, occ), L, pinned_material=True)
    ref0 = shade_env(*inputs, L)
    assert min(np.abs(ref0["nvr"]).min(), np.abs(ref0["qe"]).min()) >= MARGIN
    grad = dc._rng(ident, 9).standard_normal(p.shape).astype(F32)
    return inputs, L, grad, shade_env(*inputs, L, grad)


@functools.lru_cache(maxsize=None)
def edge_case(H, W, B=1, valid_count=None, seed=0, K=9, per_frame=False, cover=None):
    """(inputs, Env, upstream gradient, statement dict) for B frames of H x W: fully covered (cover: that share of the
    pixels, drawn); valid_count: only a frame's first pixels have a usable normal, the others a NaN one"""
    rng = np.random.default_rng([seed, H, W, B, valid_count or 0, K, int(per_frame)])
    covered = np.ones((B, H, W), bool) if cover is None else rng.random((B, H, W)) < cover
    invalid = None
    if valid_count is not None:
        invalid = (np.arange(H * W) >= valid_count).reshape(1, H, W).repeat(B, 0)
    L = draw_env(rng, B, K, per_frame)
    inputs = settled_input(rng, covered, L, invalid)
    grad = rng.standard_normal(inputs[0].shape).astype(F32)
    return inputs, L, grad, shade_env(*inputs, L, grad)


def reflect_of(inputs, L, seed=0):
    """reflect_view's case on shade_env's inputs: (positions, normals, camera, upstream gradient, statement dict)"""
    p, n = inputs[0], inputs[2]
    grad = np.random.default_rng([seed, 77]).standard_normal(p.shape).astype(F32)
    return p, n, L.camera, grad, reflect_view(p, n, L.camera, grad)
