"""deferred.shade_pbr on a CPU: the statement's vector-Jacobian products (tests/shade_pbr_cases.py) against central
differences in float64; the framework-op statement `_shade_pbr_ops` against it in float64 (1e-12) and, in float32,
within half of every bound the kernels are held to; the low-roughness case; the selects; the three C entry points'
argument checks (no GPU call is made) and the public function's errors.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import deferred_cases as dc
import lighting_cases
import lighting_f64 as lf
import shade_pbr_cases as spc
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_deferred_shade_pbr_workspace", "dirt_deferred_shade_pbr_fwd", "dirt_deferred_shade_pbr_bwd")
NAMES = spc.PIXEL_NAMES
LOW_ROUGHNESS_W = 2.33  # test_low_roughness's measured worst forward ratio, rounded up (see its docstring)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the statement's own derivatives

def _rows_inputs(point, seed=0, rows=6):
    """rows kept 0.05 away from the nl kink, the n.v kink and the clamps' ends"""
    rng = np.random.default_rng(seed)
    cam = np.array([0.25, 1.75, 2.25])
    vec = np.array([0.5, -2.5, 1.0]) if point else np.array([0.3, -0.6, -0.5])
    while True:
        p = rng.uniform(-1, 1, (rows, 3))
        nd = rng.standard_normal((rows, 3)) * rng.uniform(0.5, 2.0, (rows, 1))  # (not unit: u's Jacobian is exercised)
        c = rng.uniform(0.2, 1, (rows, 3))
        mat = np.stack([rng.uniform(0.25, 0.95, rows), rng.uniform(0.05, 0.95, rows)], -1)
        vis = rng.uniform(0.05, 1, (rows, 1))
        n, v = lf._over_length_eps(nd), lf._over_length_eps(cam - p)
        l = lf._over_length_eps((vec - p) if point else np.broadcast_to(-vec, p.shape))
        h = lf._over_length_eps(l + v)
        nl, nv, vh = lf._dot(n, l), lf._dot(n, v), lf._dot(v, h)
        if np.abs(nl).min() > 0.05 and np.abs(nv).min() > 0.05 and vh.min() > 0.05 and vh.max() < 0.95 and \
                (nl > 0).sum() >= 2 and (nl < 0).sum() >= 1:
            return p, nd, c, mat, vis, vec, rng.uniform(0.2, 1, 3), cam, rng.standard_normal((rows, 3))


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
def test_per_light_vjp_against_central_differences(point):
    p, nd, c, mat, vis, vec, lc, cam, g = _rows_inputs(point)
    ref = spc.light_rows(p, nd, c, mat, vis, g, vec, lc, cam, point)
    base = dict(p=p, nd=nd, c=c, mat=mat, vis=vis, vec=vec, lc=lc, cam=cam)

    def loss(**kw):
        a = dict(base, **kw)
        return (spc.light_rows(a["p"], a["nd"], a["c"], a["mat"], a["vis"], None, a["vec"], a["lc"], a["cam"],
                               point)["term"] * g).sum()
    for key, name, summed in (("p", "positions", False), ("nd", "normals", False), ("c", "colors", False),
                              ("mat", "material", False), ("vis", "visibility", False), ("vec", "vectors", True),
                              ("lc", "light_colors", True), ("cam", "camera", True)):
        x = base[key]
        num = np.zeros(x.shape)
        for idx in np.ndindex(*x.shape):
            hi, lo = x.copy(), x.copy()
            hi[idx] += 1e-6
            lo[idx] -= 1e-6
            num[idx] = (loss(**{key: hi}) - loss(**{key: lo})) / 2e-6
        want = ref[name].sum(0) if summed else ref[name]
        assert np.abs(num - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), name
    unlit = (ref["d"] == 0).all(-1)
    assert unlit.any() and not unlit.all()
    for name in NAMES + ("vectors", "light_colors", "camera"):
        assert np.all(ref[name][unlit] == 0), name


def _steady_case(ident, per_frame):
    """a frame's case with every valid pixel 0.05 away from the kinks under its three lights (redrawn until so)"""
    covered = dict(dc.FRAMES)[ident]
    for seed in range(200):
        rng = dc._rng(ident, 41, seed)
        L = spc.draw_lights(rng, covered.shape[0], 3, "mixed", per_frame)
        p, c, n, mat, vis = spc.random_input(rng, covered, 3, roughness=(0.25, 0.95))
        mat[..., 1] = np.clip(mat[..., 1], 0.05, 0.95)
        squeeze, rp, rn, valid, P, N, C = dc._shade_terms(p, c, n, None)
        ok = True
        for b in range(covered.shape[0]):
            vectors, _, cam = L.frame(b)
            pp, nn = P[b][valid[b]], lf._over_length_eps(N[b][valid[b]])
            v = lf._over_length_eps(np.asarray(cam, np.float64) - pp)
            ok = ok and (len(pp) == 0 or np.abs(lf._dot(nn, v)).min() > 0.05)
            for i in range(3):
                l = lf._over_length_eps((vectors[i] - pp) if L.point[i] else np.broadcast_to(-vectors[i].astype(
                    np.float64), pp.shape))
                vh = lf._dot(v, lf._over_length_eps(l + v))
                ok = ok and (len(pp) == 0 or (np.abs(lf._dot(nn, l)).min() > 0.05 and vh.min() > 0.05 and
                                              vh.max() < 0.95))
        if ok:
            return (p, c, n, mat, vis), L, rng.standard_normal(p.shape).astype(np.float32)
    raise AssertionError("no steady draw for %s" % ident)


@pytest.mark.parametrize("ident,per_frame", [("2x2-hole", False), ("1x7-block_tl", False), ("3x5x6-leak", True)])
def test_whole_statement_against_central_differences(ident, per_frame):
    """Every gradient the statement returns -- the five per-pixel inputs, positions and normals through the dilation,
    and each parameter -- against central differences of sum(pixels * grad)."""
    inputs, L, grad = _steady_case(ident, per_frame)
    ref = spc.shade_pbr(*inputs, L, grad)
    assert ref["valid"].any()
    loss = lambda out: (out["pixels"] * grad).sum()  # noqa: E731
    for i, name in enumerate(NAMES):
        x = inputs[i].astype(np.float64)
        finite = np.isfinite(x)
        num = np.zeros(x.shape)
        for idx in zip(*np.nonzero(finite)):
            vals = []
            for step in (1e-6, -1e-6):
                args = [a.astype(np.float64) for a in inputs]
                args[i][idx] += step
                vals.append(loss(spc.shade_pbr(*args, L)))
            num[idx] = (vals[0] - vals[1]) / 2e-6
        want = np.where(finite, ref[name], 0.0)
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name
        assert not np.any(ref[name][~finite])
    for name, want in ref["params"].items():
        x = np.asarray(getattr(L, name), np.float64)
        num = np.zeros(x.shape)
        for idx in np.ndindex(*x.shape):
            vals = []
            for step in (1e-6, -1e-6):
                v = x.copy()
                v[idx] += step
                M = spc.LightSet(L.vectors, L.colors, L.camera, L.ambient, L.point)
                setattr(M, name, v)  # (float64: LightSet's float32 cast bypassed)
                vals.append(loss(spc.shade_pbr(*inputs, M)))
            num[idx] = (vals[0] - vals[1]) / 2e-6
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name


# ---- `_shade_pbr_ops` against the statement

def _ops_run(inputs, L, grad, dtype, dev="cpu", fn=None, visibility=True):
    """-> (pixels, valid, {name: gradient as numpy}) of `_shade_pbr_ops` (or fn) with every gradient requested"""
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype).requires_grad_(True)  # noqa: E731
    ts = [to(a) for a in inputs]
    if not visibility:
        ts = ts[:4]
    ps = {"vectors": to(L.vectors), "colors": to(L.colors), "camera": to(L.camera)}
    if L.ambient is not None:
        ps["ambient"] = to(L.ambient)
    pixels, valid = (fn or deferred._shade_pbr_ops)(*ts[:4], ps["vectors"], ps["colors"], ps["camera"],
                                                    ps.get("ambient"), L.point, ts[4] if visibility else None)
    named = list(zip(NAMES, ts)) + [("param_" + n, p) for n, p in ps.items()]
    named = [(n, t) for n, t in named if t.numel()]
    grads = torch.autograd.grad(pixels, [t for _, t in named], torch.from_numpy(grad).to(dev).to(dtype),
                                allow_unused=True)
    out = {n: (torch.zeros_like(t) if g is None else g).detach().cpu().numpy() for (n, t), g in zip(named, grads)}
    return pixels.detach().cpu().numpy(), valid.cpu().numpy(), out


def _check_f64(inputs, L, grad, ref, tag):
    pixels, valid, grads = _ops_run(inputs, L, grad, torch.float64)
    assert valid.shape == ref["valid"].shape + (1,) and np.array_equal(valid[..., 0], ref["valid"]), tag
    assert np.array_equal(pixels[~ref["valid"]], np.zeros_like(pixels[~ref["valid"]])), tag
    assert np.all(np.abs(pixels - ref["pixels"]) <= 1e-12 * np.maximum(1.0, np.abs(ref["pixels"]))), tag
    for name in NAMES:
        if name not in grads:
            continue
        assert np.all(np.isfinite(grads[name])), (tag, name)
        assert np.abs(grads[name] - ref[name]).max() <= 1e-12 * max(1.0, np.abs(ref[name]).max()), (tag, name)
    for name, want in ref["params"].items():
        if np.size(want) == 0:
            continue
        got = grads["param_" + name].reshape(np.shape(want))
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (tag, name)


@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_ops_match_the_statement_in_float64(ident):
    inputs, L, grad, ref = spc.case(ident)
    _check_f64(inputs, L, grad, ref, ident)


@pytest.mark.parametrize("n,kinds", [(0, "mixed"), (1, "directional"), (1, "point"), (2, "mixed"), (8, "directional"),
                                     (8, "point"), (8, "mixed")])
def test_ops_light_counts_and_kinds_in_float64(n, kinds):
    for ident in ("15x17-checkerboard", "2x2-hole"):
        inputs, L, grad, ref = spc.case(ident, n, kinds)
        _check_f64(inputs, L, grad, ref, (ident, n, kinds))


@pytest.mark.parametrize("ambient", [True, False], ids=["ambient", "no_ambient"])
def test_ops_per_frame_lights_and_cameras_in_float64(ambient):
    inputs, L, grad, ref = spc.case("3x5x6-leak", 2, "mixed", True, ambient)
    assert L.vectors.shape == (3, 2, 3) and L.camera.shape == (3, 3)
    _check_f64(inputs, L, grad, ref, "per frame")
    for name in ("vectors", "colors", "camera"):  # the outer frames are all background
        assert np.all(ref["params"][name][[0, 2]] == 0) and np.abs(ref["params"][name][1]).max() > 0, name
    assert ("ambient" in ref["params"]) == ambient


def test_no_visibility_is_a_visibility_of_ones_bit_for_bit():
    inputs, L, grad, _ = spc.case("15x17-island")
    ones = inputs[:4] + (np.ones_like(inputs[4]),)
    for dtype in (torch.float64, torch.float32):
        a = _ops_run(ones, L, grad, dtype)
        b = _ops_run(ones, L, grad, dtype, visibility=False)
        assert np.array_equal(a[0], b[0])
        assert all(np.array_equal(a[2][k], b[2][k]) for k in b[2])
    ref1, ref0 = spc.shade_pbr(*ones, L, grad), spc.shade_pbr(*inputs[:4], None, L, grad)
    assert np.array_equal(ref1["pixels"], ref0["pixels"]) and np.array_equal(ref1["normals"], ref0["normals"])


def test_unbatched_statement_and_ops():
    inputs, L, grad, ref = spc.case("15x17-island")
    one = spc.shade_pbr(*(a[0] for a in inputs), L, grad[0])
    assert one["pixels"].shape == (15, 17, 3) and np.array_equal(one["pixels"], ref["pixels"][0])
    assert one["material"].shape == (15, 17, 2) and one["visibility"].shape == (15, 17, 2)
    pixels, valid, grads = _ops_run([a[0] for a in inputs], L, grad[0], torch.float64)
    assert pixels.shape == (15, 17, 3) and valid.shape == (15, 17, 1)
    assert np.abs(pixels - one["pixels"]).max() <= 1e-12
    assert np.abs(grads["material"] - one["material"]).max() <= 1e-12 * max(1.0, np.abs(one["material"]).max())


# ---- the bounds, on a CPU before any kernel is held to them

# (frame, lights, kinds, per-frame): every case tests/test_gpu_shade_pbr.py holds to the bounds
BOUND_CASES = ([(i, 2, "mixed", False) for i in dc.FRAME_IDS] +
               [("15x17-checkerboard", n, kinds, False)
                for n, kinds in ((1, "directional"), (1, "point"), (8, "directional"), (8, "point"), (8, "mixed"))] +
               [("3x5x6-leak", 2, "mixed", True), ("15x17-checkerboard", 3, "mixed", False)])


def measure(run, inputs, L, grad, ref, tag, limit):
    """The worst ratios of one run against the three bounds -> (forward, per-pixel gradients, parameter gradients);
    each is asserted against `limit`; a frame with a single valid pixel is left out of the parameter check."""
    pixels, valid, grads = run
    n, v = L.n, ref["valid"]
    assert np.array_equal(valid[..., 0], v), tag
    fwd = float((np.abs(pixels - ref["pixels"]) / spc.fwd_bound(ref, n)).max())
    assert fwd <= limit, (tag, "forward", fwd)
    worst_g = 0.0
    for name in NAMES:
        if name in grads and grads[name].size:
            r = lighting_cases.grad_ratio(grads[name], ref[name], name)
            assert r <= limit, (tag, name, r)
            worst_g = max(worst_g, r)
    worst_p = 0.0
    if v.sum() > 1:
        for name, want in ref["params"].items():
            if np.size(want):
                r = spc.param_ratio(grads["param_" + name], want, ref["absum"][name], lighting_cases.GRAD_FRAC)
                assert r <= limit, (tag, "param", name, r)
                worst_p = max(worst_p, r)
    return fwd, worst_g, worst_p


def test_float32_ops_stay_within_half_of_every_bound():
    """`_shade_pbr_ops` in float32 on the CPU against the forward bound (1 + 2 N) FWD_ATOL + FWD_RTOL scale, the
    per-pixel gradient bound GRAD_FRAC of the tensor's scale and the parameter bound GRAD_FRAC * absum: at most 0.5
    on every case the GPU test uses (frames with a single valid pixel are left out of the parameter check only).
    Measured: forward 0.230, per-pixel gradients 0.145, parameter gradients 0.097."""
    worst = [(0.0, None)] * 3
    for ident, n, kinds, per_frame in BOUND_CASES:
        inputs, L, grad, ref = spc.case(ident, n, kinds, per_frame)
        got = measure(_ops_run(inputs, L, grad, torch.float32), inputs, L, grad, ref, (ident, n, kinds), 0.5)
        worst = [max(w, (g, (ident, n, kinds)), key=lambda t: t[0]) for w, g in zip(worst, got)]
    print("float32 framework ops: forward %.3f at %s; per-pixel gradients %.3f at %s; parameter gradients %.3f at %s"
          % sum(worst, ()))


# ---- low roughness

@functools.lru_cache(maxsize=None)
def low_roughness_case():
    """15x17-no_background under two lights with roughness drawn from [0, 0.2): the clamp at R_MIN is active on part
    of it.  Random normals almost never meet a lobe this narrow, so every other pixel's normal is turned to the first
    (directional) light's half vector plus a deviate of 1.5 alpha: those pixels sit on the GGX peak, where t is small
    and D is alpha^-2 / pi.  -> (inputs, L, grad, ref)"""
    ident = "15x17-no_background"
    p, c, n, mat, vis = (a.copy() for a in spc.frame_input(ident, 2, (0.0, 0.2)))
    L = spc.light_set(ident, 2, "mixed")
    assert not L.point[0]
    rng = dc._rng(ident, 51)
    v = lf._over_length_eps(np.asarray(L.camera, np.float64) - p.astype(np.float64))
    h = lf._over_length_eps(lf._over_length_eps(-L.vectors[0].astype(np.float64)) + v)
    alpha = np.clip(mat[..., 0:1].astype(np.float64), spc.R_MIN, 1.0) ** 2
    peak = lf._over_length_eps(h + 1.5 * alpha * rng.standard_normal(h.shape))
    on = (np.arange(n[..., 0].size) % 2 == 0).reshape(n.shape[:-1])
    n[on] = peak[on].astype(np.float32)
    grad = dc._rng(ident, 9).standard_normal(p.shape).astype(np.float32)
    inputs = (p, c, n, mat, vis)
    return inputs, L, grad, spc.shade_pbr(*inputs, L, grad)


def test_low_roughness():
    """Roughness in [0, 0.2): everything finite, the gradient to a roughness below R_MIN exactly 0, and W, the worst
    forward ratio of float32 `_shade_pbr_ops` against the forward bound, recorded: W = 2.32 (CPU, this case, on
    the GGX peak; the per-pixel gradients 0.147 of theirs).  The GPU test holds the kernel's forward to
    max(1, 2 W)."""
    inputs, L, grad, ref = low_roughness_case()
    below = inputs[3][..., 0] < spc.R_MIN
    assert below.any() and not below.all()
    pixels, valid, grads = _ops_run(inputs, L, grad, torch.float32)
    assert np.all(np.isfinite(pixels)) and all(np.all(np.isfinite(g)) for g in grads.values())
    assert np.all(grads["material"][..., 0][below] == 0) and np.all(ref["material"][..., 0][below] == 0)
    assert np.abs(grads["material"][..., 0][~below]).max() > 0
    W = float((np.abs(pixels - ref["pixels"]) / spc.fwd_bound(ref, L.n)).max())
    worst_g = max(lighting_cases.grad_ratio(grads[name], ref[name], name) for name in NAMES)
    print("low roughness, float32 framework ops: forward W = %.3f of the bound, per-pixel gradients %.3f" % (W, worst_g))
    assert W <= LOW_ROUGHNESS_W  # (the recorded figure stays true)


# ---- the selects

def _one_pixel(normal, light, cam=(0.0, 0.0, 2.0), dtype=torch.float64):
    """a 1x1 frame at the origin under one directional light -> (pixels, gradients of everything)"""
    ts = [torch.tensor([[v]], dtype=dtype, requires_grad=True) for v in
          ([0.0, 0.0, 0.0], [0.5, 0.6, 0.7], list(normal), [0.5, 0.3], [0.8])]
    ps = [torch.tensor(v, dtype=dtype, requires_grad=True) for v in ([list(light)], [[1.0, 0.9, 0.8]], list(cam))]
    pixels, valid = deferred.shade_pbr(ts[0], ts[1], ts[2], ts[3], ps[0], ps[1], ps[2], None, None, ts[4])
    assert bool(valid.all())
    grads = torch.autograd.grad(pixels.sum(), ts + ps, allow_unused=True)
    return pixels.detach().numpy(), [None if g is None else g.numpy() for g in grads]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_selects(dtype):
    # the light travels along +z: l = -z, nl = -1 <= 0 -> exactly 0, every gradient exactly 0
    pixels, grads = _one_pixel((0, 0, 1), (0, 0, 1), dtype=dtype)
    assert np.all(pixels == 0) and all(g is None or np.all(g == 0) for g in grads)
    # nl exactly 0 (l orthogonal to n) is on the zero side too
    pixels, grads = _one_pixel((0, 0, 1), (1, 0, 0), dtype=dtype)
    assert np.all(pixels == 0) and all(g is None or np.all(g == 0) for g in grads)
    # a zero normal: n = 0, nl = 0, t = 0
    pixels, grads = _one_pixel((0, 0, 0), (0, 0, -1), dtype=dtype)
    assert np.all(pixels == 0) and all(g is None or np.all(np.isfinite(g)) for g in grads)
    # l = -v exactly (the camera at distance 1 on the light's axis, the surface facing the light): h = 0 and t = 0
    # with nl > 0 -> D = 0 by the select, everything finite
    pixels, grads = _one_pixel((0, 0, -1), (0, 0, 1), cam=(0.0, 0.0, 1.0), dtype=dtype)
    assert np.all(np.isfinite(pixels)) and all(g is None or np.all(np.isfinite(g)) for g in grads)
    ref = spc.shade_pbr(np.zeros((1, 1, 3)), np.array([[[0.5, 0.6, 0.7]]]), np.array([[[0.0, 0.0, -1.0]]]),
                        np.array([[[0.5, 0.3]]]), np.array([[[0.8]]]),
                        spc.LightSet([[0, 0, 1]], [[1.0, 0.9, 0.8]], [0, 0, 1], None, (False,)), np.ones((1, 1, 3)))
    assert np.abs(pixels - ref["pixels"]).max() <= 1e-6
    assert all(np.all(np.isfinite(ref[k])) for k in NAMES)


# ---- the C entry points

def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "dirt_mi355x.h")).read()
    assert all(("int %s(" % n) in header for n in NEW_SYMBOLS) and "#define DIRT_PBR_MIN_ROUGHNESS 0.045f" in header
    assert _lib.PBR_MIN_ROUGHNESS == float(np.float32(0.045)) == spc.R_MIN


def _workspace(B, H, W, n):
    size = ctypes.c_size_t(0)
    assert _lib.load().dirt_deferred_shade_pbr_workspace(B, H, W, n, ctypes.byref(size)) == _lib.DIRT_OK
    return size.value


def _args(fn, B=1, H=4, W=4, n=2, mask=0, null=(), workspace_short=0, want=("grad_positions", "grad_camera")):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    a = [p("positions"), p("colors"), p("normals"), p("material"), p("visibility"), B, H, W, p("ambient"), n, mask, 0,
         p("vectors"), p("light_colors"), 0, p("camera")]
    if fn.endswith("fwd"):
        return a + [p("pixels"), p("valid"), p("route"), None], word
    outs = ("grad_positions", "grad_colors", "grad_normals", "grad_material", "grad_visibility", "grad_ambient",
            "grad_vectors", "grad_light_colors", "grad_camera")
    size = _workspace(max(B, 0), H, W, n) if 1 <= H <= _lib.MAX_DIM and 1 <= W <= _lib.MAX_DIM and 0 <= n <= 8 else 0
    return a + [p("grad_pixels"), p("route")] + [p(o) if o in want else None for o in outs] + \
        [p("workspace"), size - workspace_short, None], word


def test_workspace_size():
    for B, H, W, n in ((1, 4, 4, 0), (1, 32, 32, 2), (2, 33, 65, 8), (0, 4, 4, 2), (3, 1, 257, 1)):
        assert _workspace(B, H, W, n) == B * ((H * W + 255) // 256) * (6 + 6 * n) * 4
    lib, size = _lib.load(), ctypes.c_size_t(0)
    assert lib.dirt_deferred_shade_pbr_workspace(1, 4, 4, 9, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert "lights" in lib.dirt_last_error().decode()
    assert lib.dirt_deferred_shade_pbr_workspace(1, 0, 4, 1, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_deferred_shade_pbr_workspace(1, 4, 4, 1, None) == _lib.DIRT_EINVAL


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    for fn in NEW_SYMBOLS[1:]:
        f = getattr(lib, fn)
        for bad, msg in ((dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=0), "height, width"),
                         (dict(H=_lib.MAX_DIM + 1), "height, width"), (dict(n=-1), "lights"), (dict(n=9), "lights"),
                         (dict(n=2, mask=4), "point_mask"), (dict(n=0, mask=1), "point_mask")):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err() and "deferred_shade_pbr" in err(), (fn, bad, err())
        # B == 0: nothing to do, whatever the pointers
        a, _keep = _args(fn, B=0, null=("positions", "pixels", "grad_pixels", "route", "vectors", "workspace"))
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, H=0, null=("positions",))
        assert f(*a) == _lib.DIRT_EINVAL and "height, width" in err(), fn
    required = {"dirt_deferred_shade_pbr_fwd": ("positions", "colors", "normals", "material", "vectors",
                                                "light_colors", "camera", "pixels", "valid", "route"),
                "dirt_deferred_shade_pbr_bwd": ("positions", "colors", "normals", "material", "vectors",
                                                "light_colors", "camera", "grad_pixels", "route")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the backward: a workspace one byte short, or missing, with a parameter gradient requested
    for bad in (dict(workspace_short=1), dict(null=("workspace",))):
        a, _keep = _args("dirt_deferred_shade_pbr_bwd", **bad)
        assert lib.dirt_deferred_shade_pbr_bwd(*a) == _lib.DIRT_EINVAL and "workspace" in err(), bad
    # ... nothing requested: no work and no error, whatever else is null
    a, _keep = _args("dirt_deferred_shade_pbr_bwd", want=(), null=("positions", "route", "workspace"))
    assert lib.dirt_deferred_shade_pbr_bwd(*a) == _lib.DIRT_OK


# ---- the public function

def test_public_surface_errors():
    assert set(deferred.__all__) == {"dilate", "shade"} and callable(deferred.shade_pbr)
    g = [torch.zeros((4, 4, 3))] * 3
    mat = torch.full((4, 4, 2), 0.5)
    lights = lambda n, lead=(): [torch.ones(lead + (n, 3))] * 2  # noqa: E731
    cam = torch.ones(3)
    with pytest.raises(ValueError, match="shade_pbr: the two light arrays hold"):
        deferred.shade_pbr(*g, mat, torch.ones((2, 3)), torch.ones((3, 3)), cam)
    with pytest.raises(ValueError, match="shade_pbr: 9 lights, at most 8"):
        deferred.shade_pbr(*g, mat, *lights(9), cam)
    with pytest.raises(ValueError, match="shade_pbr: point has 3 entries"):
        deferred.shade_pbr(*g, mat, *lights(2), cam, point=(True, False, True))
    with pytest.raises(ValueError, match="shade_pbr: the two light arrays must both be shared"):
        deferred.shade_pbr(*[torch.zeros((2, 4, 4, 3))] * 3, torch.zeros((2, 4, 4, 2)), torch.ones((2, 2, 3)),
                           torch.ones((2, 3)), cam)
    with pytest.raises(ValueError, match="shade_pbr: per-frame"):
        deferred.shade_pbr(*g, mat, *lights(2, (1,)), cam)  # per-frame lights need a batch
    with pytest.raises(ValueError, match="shade_pbr: camera_position"):
        deferred.shade_pbr(*g, mat, *lights(2), torch.ones((2, 3)))
    with pytest.raises(ValueError, match="shade_pbr: positions, colors, normals must share one shape"):
        deferred.shade_pbr(g[0], g[1], torch.zeros((4, 3, 3)), mat, *lights(1), cam)
    with pytest.raises(ValueError, match="shade_pbr: material"):
        deferred.shade_pbr(*g, torch.zeros((4, 4, 3)), *lights(1), cam)
    with pytest.raises(ValueError, match="shade_pbr: visibility"):
        deferred.shade_pbr(*g, mat, *lights(2), cam, visibility=torch.ones((4, 4, 1)))
    with pytest.raises(ValueError, match="shade_pbr: light_vectors, light_colors must be"):
        deferred.shade_pbr(*g, mat, torch.ones(3), torch.ones(3), cam)
    pixels, valid = deferred.shade_pbr(*g, mat, *lights(0), cam, ambient_color=torch.ones(3))
    assert pixels.shape == (4, 4, 3) and valid.shape == (4, 4, 1) and bool(valid.all())
    doc = " ".join(deferred.shade_pbr.__doc__.split())
    assert "read at the pixel itself" in doc and "`sample_shadow` on `dilate(positions)`" in doc


def test_statement_path_supports_double_backward():
    inputs, L, grad, ref = spc.case("15x17-hole")
    ts = [torch.from_numpy(a).double().requires_grad_(True) for a in inputs]
    vec = torch.from_numpy(L.vectors).double().requires_grad_(True)
    pixels, _ = deferred.shade_pbr(*ts[:4], vec, torch.from_numpy(L.colors).double(),
                                   torch.from_numpy(L.camera).double(), None, L.point, ts[4])
    gv, = torch.autograd.grad(pixels.square().sum(), [vec], create_graph=True)
    gg, = torch.autograd.grad(gv.sum(), [ts[3]])
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0
