"""deferred.shade_lights on a CPU: the statement's vector-Jacobian products (tests/shade_lights_cases.py) against
central differences in float64; the framework-op statement `_shade_lights_ops` against it in float64 (1e-12) and, in
float32, within half of the parameter-gradient bound GRAD_FRAC * absum that the kernels are held to; one directional
light bit for bit `_shade_ops`; the three C entry points' argument checks (no GPU call is made) and the public
function's errors.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import deferred_cases as dc
import lighting_cases
import lighting_f64 as lf
import shade_lights_cases as slc
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_deferred_shade_lights_workspace", "dirt_deferred_shade_lights_fwd",
               "dirt_deferred_shade_lights_bwd")
NAMES = ("positions", "colors", "normals")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the statement's own derivatives

def _central(f, x, g, h=1e-6):
    """d (sum f(x) * g) / dx by central differences, x a float64 array"""
    out = np.zeros(x.shape)
    for idx in np.ndindex(*x.shape):
        hi, lo = x.copy(), x.copy()
        hi[idx] += h
        lo[idx] -= h
        out[idx] = ((f(hi) - f(lo)) * g).sum() / (2 * h)
    return out


def _rows_inputs(two, seed=0, rows=6):
    """positions, normals, reflectivities, light position, colour, camera, upstream gradient: |cos| of the specular
    term at least 0.05 (away from the clamp's kink, where a central difference straddles it)"""
    rng = np.random.default_rng(seed)
    while True:
        p = rng.uniform(-1, 1, (rows, 3))
        n = rng.standard_normal((rows, 3))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        r = rng.uniform(0.2, 1, (rows, 3))
        light, lc, cam = np.array([0.5, -2.5, 1.0]), rng.uniform(0.2, 1, 3), np.array([0.25, 1.75, 2.25])
        u = lf._over_length_eps(p - light)
        _, reflected, _, view = lf._spec_terms(p, n, u, cam)
        cos = lf._dot(view, reflected)
        if np.abs(cos).min() > 0.05 and (two or (cos > 0).sum() >= 2):
            return p, n, r, light, lc, cam, rng.standard_normal((rows, 3))


@pytest.mark.parametrize("k", [1.0, 2.5, 6.0])
@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_specular_point_vjp_against_central_differences(two, k):
    p, n, r, light, lc, cam, g = _rows_inputs(two)
    vjp = slc.specular_point_vjp(p, n, r, light, lc, cam, k, two, g)
    f = lambda **kw: slc.specular_point(kw.get("p", p), kw.get("n", n), kw.get("r", r), kw.get("light", light),  # noqa: E731
                                        kw.get("lc", lc), kw.get("cam", cam), kw.get("k", k), two)
    for name, key, x in (("positions", "p", p), ("normals", "n", n), ("reflectivities", "r", r),
                         ("light_position", "light", light), ("light_color", "lc", lc), ("camera_position", "cam", cam)):
        num = _central(lambda v: f(**{key: v}), x, g)
        assert np.abs(num - vjp[name]).max() <= 1e-7 * max(1.0, np.abs(vjp[name]).max()), name
    num = ((f(k=k + 1e-6) - f(k=k - 1e-6)) * g).sum() / 2e-6
    assert abs(num - vjp["shininess"]) <= 1e-7 * max(1.0, abs(vjp["shininess"]))


def test_specular_point_vjp_kinks_and_zero_exponent():
    """Back-facing one-sided rows get exactly 0; k = 0 has slope 0 and d/dk = ln cs; cs = 0 gives d/dk = 0."""
    p, n, r, light, lc, cam, g = _rows_inputs(False, seed=1)
    u = lf._over_length_eps(p - light)
    _, reflected, _, view = lf._spec_terms(p, n, u, cam)
    back = (lf._dot(view, reflected) < 0)[:, 0]
    assert back.any() and not back.all()
    for k in (0.5, 6.0):
        only = lambda rows: slc.specular_point_vjp(p[rows], n[rows], r[rows], light, lc, cam, k, False, g[rows])  # noqa: E731
        assert np.all(slc.specular_point(p, n, r, light, lc, cam, k, False)[back] == 0)
        vb = only(back)
        for name, v in vb.items():
            if name != "reflectivities":
                assert np.all(np.asarray(v) == 0), (k, name)
    v0 = slc.specular_point_vjp(p, n, r, light, lc, cam, 0.0, True, g)
    assert np.all(v0["positions"] == 0) and np.all(v0["normals"] == 0) and np.all(v0["light_position"] == 0)
    assert np.all(np.isfinite(v0["shininess"]))


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_per_pixel_terms_sum_to_the_vjps(two, point):
    """`_light_rows` (the per-pixel terms behind absum) against lighting_f64's vjp functions and specular_point_vjp"""
    p, n, c, light, lc, cam, g = _rows_inputs(two, seed=2, rows=40)
    vec = light if point else np.array([0.7, -0.4, -0.6])
    sc = lc[::-1].copy()
    rows = slc._light_rows(p, n, c, g, vec, lc, sc, cam, 2.5, two, point)
    _, _, vjp = slc._light_fwd_vjp(p, n, c, g, vec, lc, sc, cam, 2.5, two, point)
    for name in ("vectors", "diffuse", "specular", "camera", "shininess"):
        got, want = rows[name].sum(0).reshape(np.shape(vjp[name])), np.asarray(vjp[name])
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
    for name in NAMES:
        assert np.abs(rows[name] - vjp[name]).max() <= 1e-12 * max(1.0, np.abs(vjp[name]).max()), name


@pytest.mark.parametrize("ident,per_frame", [("2x2-hole", False), ("1x7-block_tl", False), ("3x5x6-leak", True)])
def test_whole_statement_against_central_differences(ident, per_frame):
    """Every gradient shade_lights' statement returns -- the three G-buffers through the dilation, and each parameter
    -- against central differences of sum(pixels * grad), double-sided (no kink of the one-sided clamp to straddle;
    the dilation's routing is constant under a small step)."""
    inputs, L, grad, ref = slc.case(ident, 3, "mixed", per_frame, 2.5, True)
    loss = lambda out: (out["pixels"] * grad).sum()  # noqa: E731
    for i, name in enumerate(NAMES):
        x = inputs[i].astype(np.float64)
        finite = np.isfinite(x)

        def f(v, i=i):
            args = [a.astype(np.float64) for a in inputs]
            args[i] = v
            return loss(slc.shade_lights(*args, L))
        num = np.zeros(x.shape)
        for idx in zip(*np.nonzero(finite)):
            hi, lo = x.copy(), x.copy()
            hi[idx] += 1e-6
            lo[idx] -= 1e-6
            num[idx] = (f(hi) - f(lo)) / 2e-6
        want = np.where(finite, ref[name], 0.0)
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name
        assert not np.any(ref[name][~finite]) or name == "colors"
    for name, want in ref["params"].items():
        x = np.asarray(getattr(L, name), np.float64)
        num = np.zeros(x.shape)
        for idx in np.ndindex(*x.shape):
            vals = []
            for step in (1e-6, -1e-6):
                v = x.copy()
                v[idx] += step
                M = slc.LightSet(L.vectors, L.diffuse, L.specular, L.camera, L.ambient, L.shininess, L.point,
                                 L.double_sided)
                setattr(M, name, float(v) if name == "shininess" else v)  # (float64: LightSet's float32 cast bypassed)
                vals.append(loss(slc.shade_lights(*inputs, M)))
            num[idx] = (vals[0] - vals[1]) / 2e-6
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name


# ---- `_shade_lights_ops` against the statement

def _ops_run(inputs, L, grad, dtype, dev="cpu", fn=None, shininess_tensor=True):
    """-> (pixels, valid, {name: gradient as numpy}) of `_shade_lights_ops` (or fn) with every gradient requested"""
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype).requires_grad_(True)  # noqa: E731
    ts = [to(a) for a in inputs]
    ps = {"vectors": to(L.vectors), "diffuse": to(L.diffuse), "specular": to(L.specular), "camera": to(L.camera)}
    if L.ambient is not None:
        ps["ambient"] = to(L.ambient)
    k = L.shininess
    if shininess_tensor:
        k = ps["shininess"] = torch.tensor([float(L.shininess)], dtype=dtype, device=dev, requires_grad=True)
    pixels, valid = (fn or deferred._shade_lights_ops)(*ts, ps["vectors"], ps["diffuse"], ps["specular"], ps["camera"],
                                                       k, ps.get("ambient"), L.point, L.double_sided)
    wrt = ts + [p for p in ps.values() if p.numel()]
    grads = torch.autograd.grad(pixels, wrt, torch.from_numpy(grad).to(dev).to(dtype), allow_unused=True)
    out = {}
    for (name, t), g in zip(list(zip(NAMES, ts)) + [(n, p) for n, p in ps.items() if p.numel()], grads):
        out[name] = (torch.zeros_like(t) if g is None else g).detach().cpu().numpy()
    return pixels.detach().cpu().numpy(), valid.cpu().numpy(), out


def _check_f64(inputs, L, grad, ref, tag):
    pixels, valid, grads = _ops_run(inputs, L, grad, torch.float64)
    assert valid.shape == ref["valid"].shape + (1,) and np.array_equal(valid[..., 0], ref["valid"]), tag
    assert np.array_equal(pixels[~ref["valid"]], np.zeros_like(pixels[~ref["valid"]])), tag
    # (1e-12 of the value where it exceeds 1: a dilated normal is longer than 1, and its cosine^50 is large)
    assert np.all(np.abs(pixels - ref["pixels"]) <= 1e-12 * np.maximum(1.0, np.abs(ref["pixels"]))), tag
    for name in NAMES:
        assert np.all(np.isfinite(grads[name])), (tag, name)
        assert np.abs(grads[name] - ref[name]).max() <= 1e-12 * max(1.0, np.abs(ref[name]).max()), (tag, name)
    for name, want in ref["params"].items():
        if np.size(want) == 0:
            continue
        got = grads[name].reshape(np.shape(want))
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (tag, name)


@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_ops_match_the_statement_in_float64(ident):
    inputs, L, grad, ref = slc.case(ident)
    _check_f64(inputs, L, grad, ref, ident)


@pytest.mark.parametrize("n,kinds", [(0, "mixed"), (1, "directional"), (1, "point"), (2, "mixed"), (8, "directional"),
                                     (8, "point"), (8, "mixed")])
@pytest.mark.parametrize("two,shininess", [(False, 6.0), (True, 2.5), (False, 0), (True, 1), (False, 50.0)])
def test_ops_light_counts_and_options_in_float64(n, kinds, two, shininess):
    for ident in ("15x17-checkerboard", "2x2-hole"):
        inputs, L, grad, ref = slc.case(ident, n, kinds, False, shininess, two)
        _check_f64(inputs, L, grad, ref, (ident, n, kinds, two, shininess))


@pytest.mark.parametrize("ambient", [True, False], ids=["ambient", "no_ambient"])
def test_ops_per_frame_lights_and_cameras_in_float64(ambient):
    inputs, L, grad, ref = slc.case("3x5x6-leak", 2, "mixed", True, 6.0, False, ambient)
    assert L.vectors.shape == (3, 2, 3) and L.camera.shape == (3, 3)
    _check_f64(inputs, L, grad, ref, "per frame")
    for name in ("vectors", "diffuse", "specular", "camera"):  # the outer frames are all background
        assert np.all(ref["params"][name][[0, 2]] == 0) and np.abs(ref["params"][name][1]).max() > 0, name
    assert ("ambient" in ref["params"]) == ambient


def test_unbatched_statement_and_ops():
    inputs, L, grad, ref = slc.case("15x17-island")
    one = slc.shade_lights(*(a[0] for a in inputs), L, grad[0])
    assert one["pixels"].shape == (15, 17, 3) and np.array_equal(one["pixels"], ref["pixels"][0])
    pixels, valid, grads = _ops_run([a[0] for a in inputs], L, grad[0], torch.float64)
    assert pixels.shape == (15, 17, 3) and valid.shape == (15, 17, 1)
    assert np.abs(pixels - one["pixels"]).max() <= 1e-12


@pytest.mark.parametrize("ident", [i for i in dc.FRAME_IDS if not i.startswith("3x")])
def test_one_directional_light_equals_shade_ops_bit_for_bit(ident):
    """float32: N = 1 directional `_shade_lights_ops` is `_shade_ops` -- pixels, valid and the three G-buffer gradients"""
    inputs, L0, _, grad, _ = dc.shade_case(ident)
    ts = [torch.from_numpy(a).requires_grad_(True) for a in inputs]
    amb, ld, dcol, scol, cam = (torch.from_numpy(v) for v in L0.vectors())
    want = deferred._shade_ops(*ts, amb, ld, dcol, scol, cam, L0.shininess, L0.double_sided)
    got = deferred._shade_lights_ops(*ts, ld[None], dcol[None], scol[None], cam, L0.shininess, amb, None,
                                     L0.double_sided)
    assert torch.equal(want[1], got[1])
    assert np.array_equal(_bits(want[0].detach().numpy()), _bits(got[0].detach().numpy()))
    gw = torch.autograd.grad(want[0], ts, torch.from_numpy(grad))
    gg = torch.autograd.grad(got[0], ts, torch.from_numpy(grad))
    for a, b in zip(gw, gg):
        assert np.array_equal(_bits(a.numpy()), _bits(b.numpy()))
    pub = deferred.shade_lights(*ts, ld[None], dcol[None], scol[None], cam, L0.shininess, amb)
    assert np.array_equal(_bits(pub[0].detach().numpy()), _bits(want[0].detach().numpy())) and pub[1].dtype == torch.bool


# ---- the parameter-gradient bound, on a CPU before any kernel is held to it

# (frame, lights, kinds, per-frame, shininess, double-sided): every case tests/test_gpu_shade_lights.py holds to
# GRAD_FRAC * absum
BOUND_CASES = ([(i, 2, "mixed", False, 6.0, False) for i in slc.accuracy_frames()] +
               [("15x17-checkerboard", n, kinds, False, 6.0, False)
                for n, kinds in ((1, "directional"), (1, "point"), (8, "directional"), (8, "point"), (8, "mixed"))] +
               [("63x65-hole", 2, "mixed", False, k, two) for k in (0, 1, 2.5, 6, 50) for two in (False, True)] +
               [("3x5x6-leak", 2, "mixed", True, 6.0, False)])


def test_float32_ops_stay_within_half_the_parameter_bound():
    """`_shade_lights_ops` in float32 on the CPU against GRAD_FRAC * absum: at most 0.5 on every case the GPU test
    uses (the bound is the per-element contract of 1e-4 of scale applied to the sum of absolute terms; the 1x1
    frames are left out: their single pixel's specular cosine cancels)."""
    worst, worst_fwd, worst_g = (0.0, None), (0.0, None), (0.0, None)
    for ident, n, kinds, per_frame, k, two in BOUND_CASES:
        inputs, L, grad, ref = slc.case(ident, n, kinds, per_frame, k, two)
        pixels, _, grads = _ops_run(inputs, L, grad, torch.float32)
        # (the forward and G-buffer bounds of the GPU test, measured here as well; asserted there)
        v = ref["valid"]
        if v.any():
            worst_fwd = max(worst_fwd, (float((np.abs(pixels - ref["pixels"])[v] / slc.fwd_bound(ref, n)[v]).max()),
                                        (ident, n, kinds, k, two)))
        for name in NAMES:
            worst_g = max(worst_g, (lighting_cases.grad_ratio(grads[name], ref[name], name), (ident, n, kinds, k, two)))
        for name, want in ref["params"].items():
            if np.size(want) == 0:
                continue
            r = slc.param_ratio(grads[name], want, ref["absum"][name], lighting_cases.GRAD_FRAC)
            worst = max(worst, (r, (ident, n, kinds, k, two, name)))
            assert r <= 0.5, (ident, n, kinds, k, two, name, r)
    print("float32 framework ops: parameter gradients at most %.3f of GRAD_FRAC * absum, at %s" % worst)
    print("  forward at most %.3f of its bound, at %s; G-buffer gradients %.3f of theirs, at %s" % (worst_fwd + worst_g))


def test_one_pixel_frames_stay_finite_in_float32():
    for ident in [i for i in dc.FRAME_IDS if i.startswith("1x1-")]:
        inputs, L, grad, ref = slc.case(ident)
        _, _, grads = _ops_run(inputs, L, grad, torch.float32)
        assert all(np.all(np.isfinite(g)) for g in grads.values()), ident


# ---- the C entry points

def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "dirt_mi355x.h")).read()
    assert all(("int %s(" % n) in header for n in NEW_SYMBOLS) and "#define DIRT_MAX_LIGHTS 8" in header
    assert _lib.MAX_LIGHTS == 8


def _workspace(B, H, W, n):
    size = ctypes.c_size_t(0)
    assert _lib.load().dirt_deferred_shade_lights_workspace(B, H, W, n, ctypes.byref(size)) == _lib.DIRT_OK
    return size.value


def _args(fn, B=1, H=4, W=4, n=2, mask=0, null=(), workspace_short=0, want=("grad_positions", "grad_camera")):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    a = [p("positions"), p("colors"), p("normals"), B, H, W, p("ambient"), n, mask, 0, p("vectors"), p("diffuse"),
         p("specular"), 0, p("camera"), 6.0, None, 0]
    if fn.endswith("fwd"):
        return a + [p("pixels"), p("valid"), p("route"), None], word
    outs = ("grad_positions", "grad_colors", "grad_normals", "grad_ambient", "grad_vectors", "grad_diffuse",
            "grad_specular", "grad_camera", "grad_shininess")
    size = _workspace(max(B, 0), H, W, n) if 1 <= H <= _lib.MAX_DIM and 1 <= W <= _lib.MAX_DIM and 0 <= n <= 8 else 0
    return a + [p("grad_pixels"), p("route")] + [p(o) if o in want else None for o in outs] + \
        [p("workspace"), size - workspace_short, None], word


def test_workspace_size():
    assert _workspace(1, 4, 4, 0) == 7 * 4 and _workspace(1, 32, 32, 2) == 4 * 25 * 4
    assert _workspace(2, 33, 65, 8) == 2 * 9 * 79 * 4 and _workspace(0, 4, 4, 2) == 0
    lib, size = _lib.load(), ctypes.c_size_t(0)
    assert lib.dirt_deferred_shade_lights_workspace(1, 4, 4, 9, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert "lights" in lib.dirt_last_error().decode()
    assert lib.dirt_deferred_shade_lights_workspace(1, 0, 4, 1, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_deferred_shade_lights_workspace(1, 4, 4, 1, None) == _lib.DIRT_EINVAL


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
            assert msg in err(), (fn, bad, err())
        # B == 0: nothing to do, whatever the pointers
        a, _keep = _args(fn, B=0, null=("positions", "pixels", "grad_pixels", "route", "vectors", "workspace"))
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, H=0, null=("positions",))
        assert f(*a) == _lib.DIRT_EINVAL and "height, width" in err(), fn
    required = {"dirt_deferred_shade_lights_fwd": ("positions", "colors", "normals", "vectors", "diffuse", "specular",
                                                   "camera", "pixels", "valid", "route"),
                "dirt_deferred_shade_lights_bwd": ("positions", "colors", "normals", "vectors", "diffuse", "specular",
                                                   "camera", "grad_pixels", "route")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the backward: a workspace one byte short, or missing, with a parameter gradient requested
    for bad in (dict(workspace_short=1), dict(null=("workspace",))):
        a, _keep = _args("dirt_deferred_shade_lights_bwd", **bad)
        assert lib.dirt_deferred_shade_lights_bwd(*a) == _lib.DIRT_EINVAL and "workspace" in err(), bad
    # ... nothing requested: no work and no error, whatever else is null
    a, _keep = _args("dirt_deferred_shade_lights_bwd", want=(), null=("positions", "route", "workspace"))
    assert lib.dirt_deferred_shade_lights_bwd(*a) == _lib.DIRT_OK


# ---- the public function

def test_public_surface_errors():
    assert set(deferred.__all__) == {"dilate", "shade"} and callable(deferred.shade_lights)
    g = [torch.zeros((4, 4, 3))] * 3
    lights = lambda n, lead=(): [torch.ones(lead + (n, 3))] * 3  # noqa: E731
    cam = torch.ones(3)
    with pytest.raises(ValueError, match="hold"):
        deferred.shade_lights(*g, torch.ones((2, 3)), torch.ones((3, 3)), torch.ones((2, 3)), cam, 6.0)
    with pytest.raises(ValueError, match="at most 8"):
        deferred.shade_lights(*g, *lights(9), cam, 6.0)
    with pytest.raises(ValueError, match="point has 3 entries"):
        deferred.shade_lights(*g, *lights(2), cam, 6.0, point=(True, False, True))
    with pytest.raises(ValueError, match="all be shared"):
        deferred.shade_lights(*[torch.zeros((2, 4, 4, 3))] * 3, torch.ones((2, 2, 3)), torch.ones((2, 3)),
                              torch.ones((2, 3)), cam, 6.0)
    with pytest.raises(ValueError, match="per frame"):
        deferred.shade_lights(*g, *lights(2, (1,)), cam, 6.0)  # per-frame lights need a batch
    with pytest.raises(ValueError, match="camera_position"):
        deferred.shade_lights(*g, *lights(2), torch.ones((2, 3)), 6.0)
    with pytest.raises(ValueError, match="share one shape"):
        deferred.shade_lights(g[0], g[1], torch.zeros((4, 3, 3)), *lights(1), cam, 6.0)
    with pytest.raises(ValueError, match="one-element"):
        deferred.shade_lights(*g, *lights(1), cam, torch.ones(2))
    pixels, valid = deferred.shade_lights(*g, *lights(0), cam, 6.0, ambient_color=torch.ones(3))
    assert pixels.shape == (4, 4, 3) and valid.shape == (4, 4, 1) and bool(valid.all())


def test_statement_path_supports_double_backward():
    inputs, L, grad, ref = slc.case("15x17-hole")
    ts = [torch.from_numpy(a).double().requires_grad_(True) for a in inputs]
    vec = torch.from_numpy(L.vectors).double().requires_grad_(True)
    pixels, _ = deferred.shade_lights(*ts, vec, torch.from_numpy(L.diffuse).double(),
                                      torch.from_numpy(L.specular).double(), torch.from_numpy(L.camera).double(),
                                      L.shininess, None, L.point)
    gv, = torch.autograd.grad(pixels.square().sum(), [vec], create_graph=True)
    gg, = torch.autograd.grad(gv.sum(), [ts[2]])
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0
