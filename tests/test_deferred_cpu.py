"""dirt_amd.deferred on a CPU: the framework-op statements `_dilate_ops` / `_shade_ops` against the float64 statement of
record (tests/deferred_cases.py) on its table of edge frames, and against torch autograd of the chain's own glue
(tests/deferred_pipeline.py::shade) bit for bit; the four C entry points' argument checks (no GPU call is made).
"""
import ctypes

import numpy as np
import pytest
import torch

import deferred_cases as dc
import deferred_pipeline as dp
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_dilate_fwd", "dirt_dilate_bwd", "dirt_deferred_shade_fwd", "dirt_deferred_shade_bwd")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _int_grad(shape, seed=0):
    return np.random.default_rng(seed).integers(-3, 4, shape).astype(np.float32)


def _dilate_with_grad(x, mask, g):
    xt = torch.from_numpy(x).requires_grad_(True)
    y = deferred._dilate_ops(xt, None if mask is None else torch.from_numpy(mask))
    gx, = torch.autograd.grad(y, [xt], torch.from_numpy(g))
    return y.detach().numpy(), gx.numpy()


@pytest.mark.parametrize("explicit", [False, True], ids=["derived", "explicit"])
@pytest.mark.parametrize("values", ["random", "ties"])
@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_dilate_ops_match_the_statement(ident, values, explicit):
    """Forward bit-exact; backward with integer cotangents exact (the statement sums in float64, every sum of at
    most ten small integers is exact in float32 too)."""
    for C in (1, 3, 8):
        x, mask, ref, route = dc.dilate_case(ident, C, values, explicit)
        g = _int_grad(x.shape)
        got, gx = _dilate_with_grad(x, mask, g)
        assert np.array_equal(_bits(got), _bits(ref)), (ident, C)
        assert np.array_equal(gx.astype(np.float64), dc.dilate_vjp(g, route)[0]), (ident, C)


@pytest.mark.parametrize("C", [1, 3, 8])
def test_dilate_ops_special_windows(C):
    """+inf, one NaN, two NaNs (the last wins), an all -inf window, a plateau (the first maximum wins): values and
    the gradient's routing as the statement's."""
    x, mask = dc.special_windows(C)
    ref, route = dc.dilate(x, mask)
    code = dc.codes(route, C)
    assert np.isnan(ref[0, 10, 4]).all() and (code[0, 10, 4] == 5).all()  # (10, 5), after (9, 3)
    assert np.isnan(ref[0, 5, 4]).all() and (code[0, 5, 4] == 3).all()
    assert np.isposinf(ref[0, 2, 2]).all() and (code[0, 2, 2] == 1).all()
    assert np.isneginf(ref[0, 1, 13]).all() and (code[0, 1, 13] == 0).all()
    assert (ref[0, 12, 12] == 0.5).all() and (code[0, 12, 12] == 0).all()
    g = _int_grad(x.shape, 1)
    got, gx = _dilate_with_grad(x, mask, g)
    assert np.array_equal(_bits(got), _bits(ref))
    assert np.array_equal(gx.astype(np.float64), dc.dilate_vjp(g, route)[0])


def _shade_torch(fn, inputs, params, dtype, grad):
    ts = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in inputs]
    pixels, valid = fn(*ts, *params)
    grads = torch.autograd.grad(pixels, ts, torch.from_numpy(grad).to(dtype))
    return pixels.detach().numpy(), valid.numpy(), [g.numpy() for g in grads]


@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_shade_ops_match_the_statement_in_float64(ident):
    inputs, L, ref, grad, vjp = dc.shade_case(ident)
    params = [torch.from_numpy(v).double() for v in L.vectors()] + [L.shininess, L.double_sided]
    pixels, valid, grads = _shade_torch(deferred._shade_ops, inputs, params, torch.float64, grad)
    assert valid.shape == ref["valid"].shape + (1,) and np.array_equal(valid[..., 0], ref["valid"])
    assert np.array_equal(pixels[~ref["valid"]], np.zeros_like(pixels[~ref["valid"]]))
    assert np.abs(pixels - ref["pixels"]).max() <= 1e-12
    for name, g in zip(("positions", "colors", "normals"), grads):
        assert np.all(np.isfinite(g)), name
        assert np.abs(g - vjp[name]).max() <= 1e-12 * max(1.0, np.abs(vjp[name]).max()), name


@pytest.mark.parametrize("two,shininess", [(True, 6.0), (False, 0), (True, 1), (False, 2.5)])
def test_shade_ops_options_match_the_statement_in_float64(two, shininess):
    inputs, L, ref, grad, vjp = dc.shade_case("15x17-checkerboard", shininess, two)
    params = [torch.from_numpy(v).double() for v in L.vectors()] + [shininess, two]
    pixels, valid, grads = _shade_torch(deferred._shade_ops, inputs, params, torch.float64, grad)
    assert np.array_equal(valid[..., 0], ref["valid"])
    assert np.abs(pixels - ref["pixels"]).max() <= 1e-12
    for name, g in zip(("positions", "colors", "normals"), grads):
        assert np.abs(g - vjp[name]).max() <= 1e-12 * max(1.0, np.abs(vjp[name]).max()), name


@pytest.mark.parametrize("ident", [i for i in dc.FRAME_IDS if not i.startswith("3x")])
def test_shade_ops_equal_the_pipeline_glue_bit_for_bit(ident):
    """float32, the sample's constants: `_shade_ops` is tests/deferred_pipeline.py::shade -- pixels, valid and the three
    gradients under torch autograd are identical."""
    pos, col, nrm = (a[0] for a in dc.shade_input(ident))
    H, W = pos.shape[:2]
    grad = dc.shade_case(ident)[3][0]
    grey, ld, red, white = dp._constants(torch.device("cpu"))
    params = [grey, ld, red, white, dp.camera_position(H, W), 6., False]
    got = _shade_torch(deferred._shade_ops, (pos, col, nrm), params, torch.float32, grad)
    ref = _shade_torch(lambda p, c, n: dp.shade(p, c, n, H, W), (pos, col, nrm), [], torch.float32, grad)
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(_bits(got[0]), _bits(ref[0]))
    for a, b in zip(got[2], ref[2]):
        assert np.array_equal(_bits(a), _bits(b))
    # and the public entry takes the same route on a CPU
    pub = deferred.shade(torch.from_numpy(pos), torch.from_numpy(col), torch.from_numpy(nrm), *params)
    assert np.array_equal(_bits(pub[0].numpy()), _bits(ref[0])) and pub[1].dtype == torch.bool


def test_public_surface():
    import dirt_amd
    assert dirt_amd.deferred is deferred and set(deferred.__all__) == {"dilate", "shade"}
    x = torch.tensor([[[1.0], [float("-inf")], [3.0]]])  # [1, 3, 1]
    assert deferred.dilate(x).reshape(-1).tolist() == [1.0, 3.0, 3.0]
    assert deferred.dilate(x, torch.tensor([[1, 0, 0]])).reshape(-1).tolist() == [1.0, float("-inf"), 3.0]
    assert deferred.dilate(x[None]).shape == (1, 1, 3, 1)
    with pytest.raises(ValueError):
        deferred.dilate(x, torch.zeros((2, 2)))
    for bad in (torch.tensor(1.0), torch.zeros(3), torch.zeros((2, 3))):
        with pytest.raises(ValueError, match="must be"):
            deferred.dilate(bad, torch.zeros(()))
    with pytest.raises(ValueError):
        deferred.shade(torch.zeros((4, 4, 3)), torch.zeros((4, 4, 3)), torch.zeros((4, 3, 3)), *[torch.ones(3)] * 5, 6.)


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only: no signature or workspace layout changed


def _args(fn, B=1, H=4, W=4, C=3, null=()):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    lights = [p(k) for k in ("ambient", "direction", "diffuse", "specular", "camera")]
    if fn == "dirt_dilate_fwd":
        a = [p("x"), None, B, H, W, C, p("out"), p("route"), None]
    elif fn == "dirt_dilate_bwd":
        a = [p("grad_out"), p("route"), B, H, W, C, p("grad_x"), None]
    elif fn == "dirt_deferred_shade_fwd":
        a = [p("positions"), p("colors"), p("normals"), B, H, W] + lights + [6.0, 0, p("pixels"), p("valid"),
                                                                           p("route"), None]
    else:
        a = [p("positions"), p("colors"), p("normals"), B, H, W] + lights + [6.0, 0, p("grad_pixels"), p("route"),
                                                                           p("grad_positions"), None, None, None]
    return a, word


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    for fn in NEW_SYMBOLS:
        f = getattr(lib, fn)
        for bad, msg in ((dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=0), "height, width"),
                         (dict(H=_lib.MAX_DIM + 1), "height, width"), (dict(W=_lib.MAX_DIM + 1), "height, width")):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err(), (fn, bad, err())
        if "dilate" in fn:
            for C in (0, _lib.MAX_CHANNELS + 1):
                a, _keep = _args(fn, C=C)
                assert f(*a) == _lib.DIRT_EINVAL and "channels" in err(), (fn, C)
        # B == 0: nothing to do, whatever the pointers
        a, _keep = _args(fn, B=0, null=("x", "out", "route", "grad_out", "grad_x", "positions", "pixels", "grad_pixels"))
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, H=0, null=("x", "grad_out", "positions"))
        assert f(*a) == _lib.DIRT_EINVAL and "height, width" in err(), fn
    required = {"dirt_dilate_fwd": ("x", "out", "route"), "dirt_dilate_bwd": ("grad_out", "route", "grad_x"),
                "dirt_deferred_shade_fwd": ("positions", "colors", "normals", "ambient", "direction", "diffuse",
                                            "specular", "camera", "pixels", "valid", "route"),
                "dirt_deferred_shade_bwd": ("positions", "colors", "normals", "ambient", "direction", "diffuse",
                                            "specular", "camera", "grad_pixels", "route")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the shade's backward with no gradient requested: no work and no error
    a, _keep = _args("dirt_deferred_shade_bwd", null=("grad_positions", "positions", "route"))
    assert lib.dirt_deferred_shade_bwd(*a) == _lib.DIRT_OK
