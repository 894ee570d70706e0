"""Statement of record for deferred.shade_sh (dirt_amd/deferred.py, dirt_amd/csrc/shade_sh_kernels.h): numpy float64,
no torch and no code shared with either implementation.  TEST INFRASTRUCTURE ONLY.

The normals are dilated by tests/deferred_cases.py's rule under `mask` (None: the pixels where a channel is +-inf);
valid = the three dilated values are finite; route = the normals' codes from bit 0 | valid << 31.  With `normalize` the
dilated normal n is replaced by u = lighting_f64._over_length_eps(n), else used raw.  For a valid pixel, with
(x, y, z) that vector and the constants as float32 rounds them:
    Y0 = c0          Y1 = c1 y        Y2 = c1 z            Y3 = c1 x
    Y4 = c2 (x y)    Y5 = c2 (y z)    Y6 = c3 (3 z^2 - 1)  Y7 = c2 (x z)    Y8 = c4 (x^2 - y^2)
    E_c = coefficients[0,c] Y0;  E_c = E_c + coefficients[k,c] Y_k, k in index order;  pixels_c = colors_c E_c
Gradients, g the upstream gradient at valid pixels and 0 elsewhere: colors: g E; gE = g colors; coefficients[k,c]:
the sum of gE_c Y_k over the valid pixels of the frame (per-frame form [B,K,3]) or of all frames (shared [K,3]);
g_u = sum_c gE_c sum_k coefficients[k,c] grad Y_k, through lighting_f64._over_length_eps_vjp with `normalize`, then
through the dilation by deferred_cases.gather.
`absum` is, per coefficient element, the sum of the absolute per-pixel terms; `scale` serves the forward bound:
scale_c = |colors_c| sum_k |coefficients[k,c]| Yhat_k with Yhat_k = |Y_k| except the two terms that cancel, taken
uncancelled: Yhat6 = c3 (3 z^2 + 1), Yhat8 = c4 (x^2 + y^2).
"""
import functools

import numpy as np

import deferred_cases as dc
import lighting_cases
import lighting_f64 as lf
from deferred_cases import FRAMES, FRAME_IDS  # noqa: F401  (the frame table, reused)

F32 = np.float32
COUNTS = (1, 4, 9)
C0, C1, C2, C3, C4 = (float(F32(c)) for c in (0.28209479177387814, 0.4886025119029199, 1.0925484305920792,
                                              0.31539156525252005, 0.5462742152960396))


def basis(u, K):
    """u [R,3] -> (Y [R,K], Yhat [R,K], dY [R,K,3] = the gradients of Y_k with respect to u)"""
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    one, zero = np.ones_like(x), np.zeros_like(x)
    Y, Yh, dY = [C0 * one], [C0 * one], [(zero, zero, zero)]
    if K > 1:
        Y += [C1 * y, C1 * z, C1 * x]
        Yh += [np.abs(C1 * y), np.abs(C1 * z), np.abs(C1 * x)]
        dY += [(zero, C1 * one, zero), (zero, zero, C1 * one), (C1 * one, zero, zero)]
    if K > 4:
        Y += [C2 * (x * y), C2 * (y * z), C3 * (3.0 * (z * z) - 1.0), C2 * (x * z), C4 * (x * x - y * y)]
        Yh += [np.abs(C2 * (x * y)), np.abs(C2 * (y * z)), C3 * (3.0 * (z * z) + 1.0), np.abs(C2 * (x * z)),
               C4 * (x * x + y * y)]
        dY += [(C2 * y, C2 * x, zero), (zero, C2 * z, C2 * y), (zero, zero, 6.0 * C3 * z), (C2 * z, zero, C2 * x),
               (2.0 * C4 * x, -2.0 * C4 * y, zero)]
    assert len(Y) == K
    return np.stack(Y, -1), np.stack(Yh, -1), np.stack([np.stack(d, -1) for d in dY], 1)


def shade_sh(colors, normals, coefficients, mask=None, normalize=False, grad=None):
    """-> dict: pixels (float64), valid (bool [B,H,W]), route (uint32), scale; with grad also the gradients colors /
    normals / coefficients (shaped as the coefficients) and absum (so shaped too).  [H,W,3] inputs give unbatched
    results."""
    cb, squeeze = dc._batched(colors)
    nb = dc._batched(normals)[0]
    B, H, W, _ = nb.shape
    coef = np.asarray(coefficients, np.float64)
    K = coef.shape[-2]
    assert K in COUNTS and (coef.ndim == 2 or coef.shape[0] == B)
    m = np.isinf(nb).any(-1) if mask is None else (np.asarray(mask).reshape(B, H, W) != 0)
    nrm_d, rn = dc.dilate(nb, m)
    valid = np.isfinite(nrm_d).all(-1)
    N = np.where(valid[..., None], np.asarray(nrm_d, np.float64), 0.0)
    C = np.where(valid[..., None], np.asarray(cb, np.float64), 0.0)
    pixels, scale = np.zeros(N.shape), np.zeros(N.shape)
    out = {"valid": valid, "route": (rn | (valid.astype(np.uint32) << np.uint32(31))).astype(np.uint32)}
    if grad is not None:
        G = np.asarray(dc._batched(grad)[0], np.float64)
        a_nrm, a_col = np.zeros(N.shape), np.zeros(N.shape)
        g_coef, absum = np.zeros(coef.shape), np.zeros(coef.shape)
    for b in range(B):
        sel = valid[b]
        n, c = N[b][sel], C[b][sel]
        cf = coef[b] if coef.ndim == 3 else coef
        u = lf._over_length_eps(n) if normalize else n
        Y, Yh, dY = basis(u, K)
        E = cf[0] * Y[:, 0:1]
        for k in range(1, K):
            E = E + cf[k] * Y[:, k:k + 1]
        pixels[b][sel] = c * E
        scale[b][sel] = np.abs(c) * (Yh @ np.abs(cf))
        if grad is None:
            continue
        g = G[b][sel]
        a_col[b][sel] = g * E
        gE = g * c
        terms = Y[:, :, None] * gE[:, None, :]  # [R,K,3]
        at = (b,) if coef.ndim == 3 else ()
        g_coef[at] += terms.sum(0)
        absum[at] += np.abs(terms).sum(0)
        w = gE @ cf.T  # [R,K]: sum_c gE_c coefficients[k,c]
        g_u = (w[:, :, None] * dY).sum(1)
        a_nrm[b][sel] = lf._over_length_eps_vjp(n, g_u) if normalize else g_u
    out["pixels"], out["scale"] = pixels, scale
    if grad is not None:
        out["normals"] = dc.gather(a_nrm, dc.codes(rn, 3))[0]
        out["colors"], out["coefficients"], out["absum"] = a_col, g_coef, absum
    if squeeze:
        out = {k: (a if k in ("coefficients", "absum") else a[0]) for k, a in out.items()}
    return out


def fwd_bound(ref, K):
    """The lighting contract (tests/lighting_cases.py) per term and summed: K terms"""
    return K * lighting_cases.FWD_ATOL + lighting_cases.FWD_RTOL * ref["scale"]


def param_ratio(got, ref, absum, frac=lighting_cases.GRAD_FRAC):
    """worst |got - ref| / (frac * absum) over the coefficients' elements (0 / 0 counts as 0; a NaN as a failure)"""
    got, ref, absum = (np.asarray(x, np.float64).reshape(-1) for x in (got, ref, absum))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / (frac * absum))
    return float(np.inf if np.isnan(ratio).any() else ratio.max(initial=0.0))


# ---- inputs

def random_input(rng, covered, invalid=None, lengths=None):
    """(colors, normals) float32 over `covered` [B,H,W] bool: unit normals (lengths=(lo, hi): of those lengths) over a
    -inf background, colours in [0.2, 1] everywhere; `invalid` [B,H,W] bool marks covered pixels whose normal is NaN."""
    shape = covered.shape + (3,)
    n = rng.standard_normal(shape)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    if lengths is not None:
        n = n * rng.uniform(lengths[0], lengths[1], covered.shape + (1,))
    n = n.astype(F32)
    c = rng.uniform(0.2, 1.0, shape).astype(F32)
    n[~covered] = -np.inf
    if invalid is not None:
        n[invalid & covered] = np.nan
    return c, n


def draw_coefficients(rng, K, frames=None):
    """float32 coefficients in [-1, 1]: [K,3], or [frames,K,3]"""
    return rng.uniform(-1.0, 1.0, (() if frames is None else (frames,)) + (K, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def sh_input(ident, lengths=None):
    """(colors, normals) float32 [B,H,W,3] for the frame `ident` of the table"""
    return random_input(dc._rng(ident, 31, 0 if lengths is None else 1), dict(FRAMES)[ident], None, lengths)


# ---- references, computed once per process and shared by the tests (treat as read-only)

@functools.lru_cache(maxsize=None)
def case(ident, K=9, per_frame=False, explicit=False, normalize=False):
    """(colors, normals, coefficients, mask or None, upstream gradient float32, statement dict with gradients) for one
    frame of the table; with normalize the normals have lengths 0.3 .. 1.5"""
    covered = dict(FRAMES)[ident]
    colors, normals = sh_input(ident, (0.3, 1.5) if normalize else None)
    coef = draw_coefficients(dc._rng(ident, 32, K, int(per_frame)), K, covered.shape[0] if per_frame else None)
    mask = dc.explicit_mask(ident, covered) if explicit else None
    grad = dc._rng(ident, 9).standard_normal(colors.shape).astype(F32)
    return colors, normals, coef, mask, grad, shade_sh(colors, normals, coef, mask, normalize, grad)
