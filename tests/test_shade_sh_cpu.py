"""deferred.shade_sh on a CPU: the statement's gradients (tests/shade_sh_cases.py) against central differences in
float64; the framework-op statement `_shade_sh_ops` against it in float64 (1e-12) on every frame of the table and, in
float32, within half of each bound the kernels are held to; the public function's errors; the three C entry points'
argument checks (no GPU call is made).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import deferred_cases as dc
import lighting_cases
import shade_sh_cases as shc
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_deferred_shade_sh_workspace", "dirt_deferred_shade_sh_fwd", "dirt_deferred_shade_sh_bwd")
NAMES = ("colors", "normals", "coefficients")
# (K, per-frame coefficients, explicit mask, normalize): every value of each, on every frame
VARIANTS = [(9, False, False, False), (4, True, True, True), (1, False, True, False), (9, True, False, True),
            (4, False, False, False), (1, True, False, True), (9, False, True, True)]


def _ops_run(colors, normals, coef, mask, normalize, grad, dtype, fn=None):
    """-> (pixels, valid, {name: gradient as numpy}) of `_shade_sh_ops` (or fn) with every gradient requested"""
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)  # noqa: E731
    ts = [to(colors), to(normals), to(coef)]
    m = None if mask is None else torch.from_numpy(mask)
    pixels, valid = (fn or deferred._shade_sh_ops)(*ts, m, normalize)
    grads = torch.autograd.grad(pixels, ts, torch.from_numpy(grad).to(dtype), allow_unused=True)
    out = {n: (torch.zeros_like(t) if g is None else g).detach().numpy() for n, t, g in zip(NAMES, ts, grads)}
    return pixels.detach().numpy(), valid.numpy(), out


@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_ops_match_the_statement_in_float64(ident):
    for K, per_frame, explicit, normalize in VARIANTS:
        colors, normals, coef, mask, grad, ref = shc.case(ident, K, per_frame, explicit, normalize)
        tag = (ident, K, per_frame, explicit, normalize)
        pixels, valid, grads = _ops_run(colors, normals, coef, mask, normalize, grad, torch.float64)
        v = ref["valid"]
        assert valid.dtype == np.bool_ and valid.shape == v.shape + (1,) and np.array_equal(valid[..., 0], v), tag
        assert np.array_equal(pixels[~v], np.zeros_like(pixels[~v])), tag
        assert np.all(np.abs(pixels - ref["pixels"]) <= 1e-12 * np.maximum(1.0, np.abs(ref["pixels"]))), tag
        for name in NAMES:
            assert np.all(np.isfinite(grads[name])), (tag, name)
            assert np.abs(grads[name] - ref[name]).max() <= 1e-12 * max(1.0, np.abs(ref[name]).max()), (tag, name)
        assert not np.any(grads["colors"][~v]), tag  # an invalid pixel carries no gradient
        if ident.endswith("all_background") and not explicit:
            assert not v.any() and not any(np.any(g) for g in grads.values()), tag


def test_per_frame_coefficients_do_not_leak_across_frames():
    colors, normals, coef, mask, grad, ref = shc.case("3x5x6-leak", 9, True)
    assert coef.shape == (3, 9, 3) and not np.any(ref["coefficients"][[0, 2]]) and np.any(ref["coefficients"][1])
    shared = shc.case("3x5x6-leak", 9, False)[5]
    assert shared["coefficients"].shape == (9, 3)


def test_unbatched_statement_and_ops():
    colors, normals, coef, mask, grad, ref = shc.case("15x17-island", 9, False, False, True)
    one = shc.shade_sh(colors[0], normals[0], coef, None, True, grad[0])
    assert one["pixels"].shape == (15, 17, 3) and np.array_equal(one["pixels"], ref["pixels"][0])
    assert np.array_equal(one["coefficients"], ref["coefficients"])
    pixels, valid, grads = _ops_run(colors[0], normals[0], coef, None, True, grad[0], torch.float64)
    assert pixels.shape == (15, 17, 3) and valid.shape == (15, 17, 1)
    assert np.abs(pixels - one["pixels"]).max() <= 1e-12
    assert np.abs(grads["normals"] - one["normals"]).max() <= 1e-12 * max(1.0, np.abs(one["normals"]).max())


# ---- the statement's own derivatives

@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("ident,K,per_frame,explicit", [
    ("2x2-hole", 9, False, False), ("1x7-block_tl", 4, False, True), ("3x5x6-leak", 9, True, False),
    ("2x2-island", 1, False, False)])
def test_statement_against_central_differences(ident, K, per_frame, explicit, normalize):
    """Every gradient the statement returns -- the colours, the normals through the normalisation and the dilation,
    the coefficients -- against central differences of sum(pixels * grad) (the routing is constant under the step)."""
    colors, normals, coef, mask, grad, ref = shc.case(ident, K, per_frame, explicit, normalize)
    inputs = {"colors": colors.astype(np.float64), "normals": normals.astype(np.float64),
              "coefficients": coef.astype(np.float64)}

    def loss(**kw):
        a = dict(inputs, **kw)
        return (shc.shade_sh(a["colors"], a["normals"], a["coefficients"], mask, normalize)["pixels"] * grad).sum()
    for name, x in inputs.items():
        finite = np.isfinite(x)
        num = np.zeros(x.shape)
        for idx in zip(*np.nonzero(finite)):
            hi, lo = x.copy(), x.copy()
            hi[idx] += 1e-6
            lo[idx] -= 1e-6
            num[idx] = (loss(**{name: hi}) - loss(**{name: lo})) / 2e-6
        want = np.where(finite, ref[name], 0.0)
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name
        assert not np.any(ref[name][~finite]) or name == "colors"


def test_statement_zero_normal_takes_the_subgradient():
    """normalize at n = 0 with bands 0-1: u = 0, the pixel is colors * coefficients[0] * c0, and the normal's gradient
    is g_u / eps (with band 2, Y6 = -c3 at u = 0 adds its term to the pixel)"""
    colors, normals, coef, _, grad, _ = shc.case("2x2-no_background", 4, False, False, True)
    normals = normals.copy()
    normals[0, 1, 1] = 0.0
    ref = shc.shade_sh(colors, normals, coef, None, True, grad)
    assert ref["valid"][0, 1, 1]
    want = colors[0, 1, 1].astype(np.float64) * coef[0].astype(np.float64) * shc.C0
    assert np.abs(ref["pixels"][0, 1, 1] - want).max() <= 1e-15
    gE = grad[0, 1, 1].astype(np.float64) * colors[0, 1, 1]
    c = coef.astype(np.float64)
    g_u = shc.C1 * np.array([gE @ c[3], gE @ c[1], gE @ c[2]])
    assert np.all(np.isfinite(ref["normals"])) and np.allclose(ref["normals"][0, 1, 1], g_u / 1e-12, rtol=1e-12)
    coef9 = shc.case("2x2-no_background", 9, False, False, True)[2]
    ref9 = shc.shade_sh(colors, normals, coef9, None, True, grad)
    c9 = coef9.astype(np.float64)
    want9 = colors[0, 1, 1].astype(np.float64) * (c9[0] * shc.C0 - c9[6] * shc.C3)
    assert np.abs(ref9["pixels"][0, 1, 1] - want9).max() <= 1e-15


# ---- the bounds, on a CPU before any kernel is held to them

# every (frame, K, per-frame, explicit mask, normalize) tests/test_gpu_shade_sh.py holds to the statement
BOUND_CASES = ([(i, 9, False, False, False) for i in dc.FRAME_IDS] +
               [(i, K, pf, False, nz) for i in ("15x17-checkerboard", "3x5x6-leak") for K in shc.COUNTS
                for pf in (False, True) for nz in (False, True)] +
               [("63x65-block_tl", 9, False, True, False), ("63x65-block_tl", 9, False, True, True)])


def test_float32_ops_stay_within_half_of_each_bound():
    """`_shade_sh_ops` in float32 on the CPU: forward within half of K * FWD_ATOL + FWD_RTOL * scale, the G-buffer
    gradients within half of grad_ratio's bound, the coefficients' within half of GRAD_FRAC * absum -- no frame of the
    table left out."""
    worst = {"forward": (0.0, None), "gbuffers": (0.0, None), "coefficients": (0.0, None)}
    for tag in BOUND_CASES:
        ident, K, per_frame, explicit, normalize = tag
        colors, normals, coef, mask, grad, ref = shc.case(*tag)
        pixels, valid, grads = _ops_run(colors, normals, coef, mask, normalize, grad, torch.float32)
        v = ref["valid"]
        assert np.array_equal(valid[..., 0], v), tag
        if v.any():
            r = float((np.abs(pixels - ref["pixels"])[v] / shc.fwd_bound(ref, K)[v]).max())
            worst["forward"] = max(worst["forward"], (r, tag))
            assert r <= 0.5, (tag, r)
        for name in NAMES[:2]:
            r = lighting_cases.grad_ratio(grads[name], ref[name], name)
            worst["gbuffers"] = max(worst["gbuffers"], (r, tag))
            assert r <= 0.5, (tag, name, r)
        r = shc.param_ratio(grads["coefficients"], ref["coefficients"], ref["absum"])
        worst["coefficients"] = max(worst["coefficients"], (r, tag))
        assert r <= 0.5, (tag, r)
    for name, (r, tag) in worst.items():
        print("float32 framework ops: %s at most %.4f of the bound, at %s" % (name, r, tag))


# ---- the public function

def test_public_surface_errors():
    g = torch.zeros((4, 4, 3))
    coef = lambda K, lead=(): torch.ones(lead + (K, 3))  # noqa: E731
    assert callable(deferred.shade_sh) and "shade_sh(" in deferred.__doc__
    for K in (0, 2, 3, 5, 8, 10, 16):
        with pytest.raises(ValueError, match="1, 4 or 9"):
            deferred.shade_sh(g, g, coef(K))
    with pytest.raises(ValueError, match="share one shape"):
        deferred.shade_sh(g, torch.zeros((4, 3, 3)), coef(9))
    with pytest.raises(ValueError, match="share one shape"):
        deferred.shade_sh(torch.zeros((4, 4, 4)), torch.zeros((4, 4, 4)), coef(9))
    with pytest.raises(ValueError, match="share one shape"):
        deferred.shade_sh(torch.zeros((4, 3)), torch.zeros((4, 3)), coef(9))
    with pytest.raises(ValueError, match=r"\[K, 3\] or \[B, K, 3\]"):
        deferred.shade_sh(g, g, torch.ones((9, 4)))
    with pytest.raises(ValueError, match=r"\[K, 3\] or \[B, K, 3\]"):
        deferred.shade_sh(g, g, torch.ones(27))
    with pytest.raises(ValueError, match="per-frame"):
        deferred.shade_sh(g, g, coef(9, (1,)))  # a per-frame form without a batch
    with pytest.raises(ValueError, match="per-frame"):
        deferred.shade_sh(g[None].repeat(2, 1, 1, 1), g[None].repeat(2, 1, 1, 1), coef(4, (3,)))
    with pytest.raises(ValueError, match="mask of shape"):
        deferred.shade_sh(g, g, coef(9), mask=torch.ones((4, 3)))
    with pytest.raises(ValueError, match="mask of shape"):
        deferred.shade_sh(g[None], g[None], coef(9), mask=torch.ones((4, 4)))
    pixels, valid = deferred.shade_sh(g + 1.0, g, coef(1))
    assert pixels.shape == (4, 4, 3) and valid.shape == (4, 4, 1) and valid.dtype == torch.bool and bool(valid.all())
    assert torch.allclose(pixels, torch.full_like(pixels, shc.C0))
    pixels, valid = deferred.shade_sh((g + 1.0).tolist(), g.tolist(), coef(4).tolist(), normalize=True)
    assert torch.allclose(pixels, torch.full_like(pixels, shc.C0))


def test_statement_path_supports_double_backward():
    colors, normals, coef, mask, grad, ref = shc.case("15x17-hole", 9, False, False, True)
    ts = [torch.from_numpy(a).double().requires_grad_(True) for a in (colors, normals, coef)]
    pixels, _ = deferred.shade_sh(*ts, normalize=True)
    assert "_ShadeShFn" not in pixels.grad_fn.name()
    gc, = torch.autograd.grad(pixels.square().sum(), [ts[2]], create_graph=True)
    gg, = torch.autograd.grad(gc.sum(), [ts[1]])
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0


# ---- the C entry points

def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "dirt_mi355x.h")).read()
    assert all(("int %s(" % n) in header for n in NEW_SYMBOLS) and "#define DIRT_MAX_SH_COEFFS 9" in header
    assert _lib.MAX_SH_COEFFS == 9


def _workspace(B, H, W, K):
    size = ctypes.c_size_t(0)
    assert _lib.load().dirt_deferred_shade_sh_workspace(B, H, W, K, ctypes.byref(size)) == _lib.DIRT_OK
    return size.value


def test_workspace_size():
    for B, H, W, K in ((1, 4, 4, 1), (1, 32, 32, 4), (2, 33, 65, 9), (0, 4, 4, 9), (3, 1, 257, 4), (1, 512, 513, 9)):
        assert _workspace(B, H, W, K) == B * -(-H * W // 256) * 3 * K * 4
    lib, size = _lib.load(), ctypes.c_size_t(0)
    for K in (0, 2, 3, 5, 8, 10, -1):
        assert lib.dirt_deferred_shade_sh_workspace(1, 4, 4, K, ctypes.byref(size)) == _lib.DIRT_EINVAL
        assert "coefficients" in lib.dirt_last_error().decode()
    assert lib.dirt_deferred_shade_sh_workspace(1, 0, 4, 9, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_deferred_shade_sh_workspace(-1, 4, 4, 9, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_deferred_shade_sh_workspace(1, 4, 4, 9, None) == _lib.DIRT_EINVAL


def _args(fn, B=1, H=4, W=4, K=9, null=(), workspace_short=0, want=("grad_colors", "grad_coefficients")):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    if fn.endswith("fwd"):
        return [p("colors"), p("normals"), p("mask"), B, H, W, K, 0, p("coefficients"), 0, p("pixels"), p("valid"),
                p("route"), None], word
    ok = 1 <= H <= _lib.MAX_DIM and 1 <= W <= _lib.MAX_DIM and K in (1, 4, 9)
    size = _workspace(max(B, 0), H, W, K) if ok else 0
    outs = ("grad_colors", "grad_normals", "grad_coefficients")
    return [p("colors"), p("normals"), B, H, W, K, 0, p("coefficients"), 1, p("grad_pixels"), p("route")] + \
        [p(o) if o in want else None for o in outs] + [p("workspace"), size - workspace_short, None], word


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    for fn in NEW_SYMBOLS[1:]:
        f = getattr(lib, fn)
        for bad, msg in ((dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=0), "height, width"),
                         (dict(H=_lib.MAX_DIM + 1), "height, width"), (dict(W=_lib.MAX_DIM + 1), "height, width"),
                         (dict(K=0), "coefficients"), (dict(K=2), "coefficients"), (dict(K=10), "coefficients"),
                         (dict(K=-4), "coefficients")):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err(), (fn, bad, err())
        # B == 0: nothing to do, whatever the pointers
        a, _keep = _args(fn, B=0, null=("colors", "pixels", "grad_pixels", "route", "coefficients", "workspace"))
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, H=0, null=("colors",))
        assert f(*a) == _lib.DIRT_EINVAL and "height, width" in err(), fn
    required = {"dirt_deferred_shade_sh_fwd": ("colors", "normals", "coefficients", "pixels", "valid", "route"),
                "dirt_deferred_shade_sh_bwd": ("colors", "normals", "coefficients", "grad_pixels", "route")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the backward: a workspace one byte short, or missing, with the coefficients' gradient requested
    for bad in (dict(workspace_short=1), dict(null=("workspace",))):
        a, _keep = _args("dirt_deferred_shade_sh_bwd", **bad)
        assert lib.dirt_deferred_shade_sh_bwd(*a) == _lib.DIRT_EINVAL and "workspace" in err(), bad
    # ... nothing requested: no work and no error, whatever else is null
    a, _keep = _args("dirt_deferred_shade_sh_bwd", want=(), null=("colors", "route", "workspace"))
    assert lib.dirt_deferred_shade_sh_bwd(*a) == _lib.DIRT_OK
