"""Statement of record for the deferred-shading stage (dirt_amd/deferred.py, dirt_amd/csrc/deferred_kernels.h), and
its table of edge frames.  numpy only, float64 arithmetic, no torch and no code shared with either implementation.
TEST INFRASTRUCTURE ONLY.

Dilation: out[p, c] = mask[p] ? max of x[., c] over the 3x3 window around p clipped to its frame : x[p, c], with
mask = "any channel of x[p] is +-inf" when none is given.  The max is the framework's CPU max_pool2d(x, 3, stride=1,
padding=1): the window is scanned in row-major order from its first element and the running value replaced when
v > m or isnan(v) -- the first maximum wins ties, a NaN gives NaN (the last NaN wins), an all -inf window picks its
first element.  route holds a 4-bit code per channel from bit 0: 0..8 = the winner's window position
(dy + 1) * 3 + (dx + 1), 15 = not dilated (unused nibbles 0).
Backward (`gather`): grad_x[p, c] = (code(p, c) == 15 ? g[p, c] : 0) + the g[q, c] of the window positions q around
p, in row-major order and including p, whose code for c points back at p (code(q, c) == 8 - k for q at position k).

Shade: bg = any channel of positions[p] is +-inf; positions and normals dilated under bg; valid = the six dilated
values are finite; pixels = valid ? diffuse_directional + specular_directional + colors * ambient : 0, composed from
tests/lighting_f64.py; route = positions' codes | normals' codes << 12 | valid << 31.  The lighting adjoints (zero at
invalid pixels) are routed through the dilation by `gather`.
"""
import functools

import numpy as np

import lighting_f64

F32 = np.float32
OWN = 15


def _batched(x):
    x = np.asarray(x)
    return (x[None], True) if x.ndim == 3 else (x, False)


def dilate(x, mask=None):
    """x [H,W,C] or [B,H,W,C] (any float dtype, kept: no arithmetic touches the values) -> (out, route uint32)"""
    xb, squeeze = _batched(x)
    B, H, W, C = xb.shape
    m = np.isinf(xb).any(-1) if mask is None else (np.asarray(mask).reshape(B, H, W) != 0)
    out = xb.copy()
    route = np.full((B, H, W), sum(OWN << (4 * c) for c in range(C)), np.uint32)
    for b in range(B):
        for y in range(H):
            for x0 in range(W):
                if not m[b, y, x0]:
                    continue
                best, code = None, None
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x0 + dx
                        if yy < 0 or yy >= H or xx < 0 or xx >= W:
                            continue
                        k = (dy + 1) * 3 + (dx + 1)
                        v = xb[b, yy, xx]
                        if best is None:
                            best, code = v.copy(), np.full(C, k)
                        else:
                            with np.errstate(invalid="ignore"):
                                take = (v > best) | np.isnan(v)
                            best[take] = v[take]
                            code[take] = k
                out[b, y, x0] = best
                route[b, y, x0] = sum(int(code[c]) << (4 * c) for c in range(C))
    return (out[0], route[0]) if squeeze else (out, route)


def codes(route, n, shift=0):
    """[..., n] codes of a route word"""
    route = np.asarray(route).astype(np.int64)
    return np.stack([(route >> (shift + 4 * c)) & 15 for c in range(n)], -1)


def gather(a, code):
    """a [B,H,W,C] float64 cotangents of the dilated values, code [B,H,W,C] -> (gradient of the undilated values,
    sum of the absolute routed terms): own term first, then the window positions in row-major order."""
    a = np.asarray(a, np.float64)
    B, H, W, C = a.shape
    gx = np.where(code == OWN, a, 0.0)
    ab = np.abs(gx)
    for k in range(9):
        dy, dx = k // 3 - 1, k % 3 - 1
        ys, yq = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
        xs, xq = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
        term = np.where(code[:, yq, xq] == 8 - k, a[:, yq, xq], 0.0)  # q = p + (dy, dx) sees p at 8 - k
        gx[:, ys, xs] += term
        ab[:, ys, xs] += np.abs(term)
    return gx, ab


def dilate_vjp(grad, route):
    """-> (grad_x float64, sum of |routed terms|), shaped as grad"""
    gb, squeeze = _batched(grad)
    rb = np.asarray(route).reshape(gb.shape[:-1])
    gx, ab = gather(gb, codes(rb, gb.shape[-1]))
    return (gx[0], ab[0]) if squeeze else (gx, ab)


class Lights:
    """The parameters of one shade call (float32 values, as both implementations receive them)."""

    def __init__(self, ambient=(0.2, 0.2, 0.2), direction=(1.0, -0.3, -0.5), diffuse=(1.0, 0.0, 0.0),
                 specular=(1.0, 1.0, 1.0), camera=(0.25, 1.75, 2.25), shininess=6.0, double_sided=False):
        d = np.asarray(direction, np.float64)
        self.ambient, self.diffuse, self.specular = (np.asarray(v, F32) for v in (ambient, diffuse, specular))
        self.direction, self.camera = (d / np.linalg.norm(d)).astype(F32), np.asarray(camera, F32)
        self.shininess, self.double_sided = shininess, double_sided

    def vectors(self):
        return [self.ambient, self.direction, self.diffuse, self.specular, self.camera]


def _shade_terms(positions, colors, normals, L):
    pb, squeeze = _batched(positions)
    cb, nb = _batched(colors)[0], _batched(normals)[0]
    bg = np.isinf(pb).any(-1)
    pos_d, rp = dilate(pb, bg)
    nrm_d, rn = dilate(nb, bg)
    valid = np.isfinite(pos_d).all(-1) & np.isfinite(nrm_d).all(-1)
    v = valid[..., None]
    P, N, Cc = (np.where(v, np.asarray(t, np.float64), 0.0) for t in (pos_d, nrm_d, cb))
    return squeeze, rp, rn, valid, P, N, Cc


def shade(positions, colors, normals, L):
    """-> dict: pixels (float64), valid (bool, [..., H, W]), route (uint32), and ambient / diffuse / specular, the
    three terms of pixels (for the per-term forward bound)"""
    squeeze, rp, rn, valid, P, N, Cc = _shade_terms(positions, colors, normals, L)
    v = valid[..., None]
    ambient = Cc * np.asarray(L.ambient, np.float64)
    diffuse = lighting_f64.diffuse_directional(N, Cc, L.direction, L.diffuse, L.double_sided)
    specular = lighting_f64.specular_directional(P, N, Cc, L.direction, L.specular, L.camera, L.shininess,
                                                 L.double_sided)
    out = {"pixels": np.where(v, diffuse + specular + ambient, 0.0), "valid": valid,
           "route": (rp | (rn << np.uint32(12)) | (valid.astype(np.uint32) << np.uint32(31))).astype(np.uint32),
           "ambient": np.where(v, ambient, 0.0), "diffuse": np.where(v, diffuse, 0.0),
           "specular": np.where(v, specular, 0.0)}
    return {k: a[0] for k, a in out.items()} if squeeze else out


def shade_vjp(positions, colors, normals, L, grad):
    """-> dict of d (sum pixels * grad) / d {positions, colors, normals} (float64)"""
    squeeze, rp, rn, valid, P, N, Cc = _shade_terms(positions, colors, normals, L)
    v = valid[..., None]
    g = np.where(v, np.asarray(_batched(grad)[0], np.float64), 0.0)
    dv = lighting_f64.diffuse_directional_vjp(N, Cc, L.direction, L.diffuse, L.double_sided, g)
    sv = lighting_f64.specular_directional_vjp(P, N, Cc, L.direction, L.specular, L.camera, L.shininess,
                                               L.double_sided, g)
    a_col = np.where(v, dv["colors"] + sv["reflectivities"] + g * np.asarray(L.ambient, np.float64), 0.0)
    a_pos = np.where(v, sv["positions"], 0.0)
    a_nrm = np.where(v, dv["normals"] + sv["normals"], 0.0)
    out = {"positions": gather(a_pos, codes(rp, 3))[0], "colors": a_col, "normals": gather(a_nrm, codes(rn, 3))[0]}
    return {k: a[0] for k, a in out.items()} if squeeze else out


# ---- the table of edge frames: the covered region of a [B, H, W] batch (True = covered)

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (15, 17), (63, 65), (16, 256)]


def _block(H, W, top, left):
    """a covered block of about half the frame touching the given corner (and so two edges)"""
    m = np.zeros((H, W), bool)
    h, w = (H + 1) // 2, (W + 1) // 2
    m[(slice(0, h) if top else slice(H - h, H)), (slice(0, w) if left else slice(W - w, W))] = True
    return m


def _hole(H, W):
    m = np.ones((H, W), bool)
    m[H // 2, W // 2] = False
    return m


def _checker(H, W):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0


LAYOUTS = {
    "block_tl": lambda H, W: _block(H, W, True, True), "block_tr": lambda H, W: _block(H, W, True, False),
    "block_bl": lambda H, W: _block(H, W, False, True), "block_br": lambda H, W: _block(H, W, False, False),
    "hole": _hole, "island": lambda H, W: ~_hole(H, W),
    "all_background": lambda H, W: np.zeros((H, W), bool), "no_background": lambda H, W: np.ones((H, W), bool),
    "checkerboard": _checker,
}


def frames():
    """[(id, covered [B,H,W] bool)]: every layout at every size, and the three-frame batch whose outer frames are
    all background and whose middle frame is fully covered (nothing may leak across frames)."""
    out = [("%dx%d-%s" % (H, W, name), fn(H, W)[None]) for H, W in SIZES for name, fn in LAYOUTS.items()]
    out.append(("3x5x6-leak", np.stack([np.zeros((5, 6), bool), np.ones((5, 6), bool), np.zeros((5, 6), bool)])))
    return out


FRAMES = frames()
FRAME_IDS = [f[0] for f in FRAMES]


def _rng(ident, *extra):
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(ident))] + list(extra))


def dilate_input(ident, covered, C, values="random"):
    """x [B,H,W,C] float32: -inf on the background; on the covered region normal deviates ('random'), or small
    integers with constant runs ('ties': equal maxima in most windows).  The leak batch's covered frame holds
    large values."""
    rng = _rng(ident, C, len(values))
    shape = covered.shape + (C,)
    if values == "ties":
        x = rng.integers(-1, 2, shape).astype(F32)
        x[..., ::2, :, :] = x[..., ::2, :1, :]  # even rows constant
    else:
        x = rng.standard_normal(shape).astype(F32)
    if ident.endswith("leak"):
        x = x + F32(1000.0)
    x[~covered] = -np.inf
    return x


def explicit_mask(ident, covered):
    """A mask independent of the values: about half the pixels, covered or not."""
    return (_rng(ident, 77).random(covered.shape) < 0.5).astype(np.uint8)


def special_windows(C):
    """(x [1,15,17,C] float32, mask uint8) with, around separate masked pixels: a +inf next to finite values, one NaN,
    two NaNs (in different channels' scan positions), an all -inf window, and a constant plateau."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 15, 17, C)).astype(F32)
    mask = np.zeros((1, 15, 17), np.uint8)
    x[0, 1, 2] = np.inf                       # +inf in the windows of (2, 2), (1, 1) ...
    x[0, 5, 3] = np.nan                       # one NaN
    x[0, 9, 3], x[0, 10, 5] = np.nan, np.nan  # two NaNs in the window of (10, 4): the last one wins
    x[0, 0:3, 12:15] = -np.inf                # the window of (1, 13) is all -inf
    x[0, 10:14, 10:15] = 0.5                  # plateau: the first maximum wins
    for y, x0 in ((2, 2), (1, 1), (5, 4), (4, 3), (10, 4), (9, 4), (1, 13), (0, 12), (12, 12), (11, 11), (5, 3)):
        mask[0, y, x0] = 1
    return x, mask


@functools.lru_cache(maxsize=None)
def shade_input(ident):
    """(positions, colors, normals) float32 [B,H,W,3] for the frame `ident`: random unit normals, positions at least
    0.5 away from Lights().camera, -inf background in positions and normals, colours in [0.2, 1] everywhere."""
    covered = dict(FRAMES)[ident]
    rng = _rng(ident, 3)
    shape = covered.shape + (3,)
    n = rng.standard_normal(shape)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    p = rng.uniform(-1.0, 1.0, shape).astype(F32)  # |camera - p| >= 0.75 - ... : the camera is at (.25, 1.75, 2.25)
    c = rng.uniform(0.2, 1.0, shape).astype(F32)
    assert np.linalg.norm(np.asarray(Lights().camera, np.float64) - p, axis=-1).min() >= 0.5
    p[~covered] = -np.inf
    n[~covered] = -np.inf
    return p, c, n


# ---- references, computed once per process and shared by the tests (treat as read-only)

@functools.lru_cache(maxsize=None)
def dilate_case(ident, C, values, explicit):
    """(x, mask or None, out, route) of the statement for one frame of the table"""
    covered = dict(FRAMES)[ident]
    x = dilate_input(ident, covered, C, values)
    mask = explicit_mask(ident, covered) if explicit else None
    out, route = dilate(x, mask)
    return x, mask, out, route


@functools.lru_cache(maxsize=None)
def shade_case(ident, shininess=6.0, double_sided=False):
    """(inputs, Lights, forward dict, upstream gradient float32, vjp dict) of the statement for one frame"""
    inputs = shade_input(ident)
    L = Lights(shininess=shininess, double_sided=double_sided)
    grad = _rng(ident, 9).standard_normal(inputs[0].shape).astype(F32)
    return inputs, L, shade(*inputs, L), grad, shade_vjp(*inputs, L, grad)


def shade_fwd_bound(ref):
    """The lighting contract (tests/lighting_cases.py) applied per term and summed"""
    import lighting_cases
    return 3 * lighting_cases.FWD_ATOL + lighting_cases.FWD_RTOL * (
        np.abs(ref["ambient"]) + np.abs(ref["diffuse"]) + np.abs(ref["specular"]))
