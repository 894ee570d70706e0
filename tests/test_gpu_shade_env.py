"""The fused reflect_view and shade_env kernels (dirt_amd/csrc/shade_env_kernels.h through dirt_amd.deferred) against
the float64 statement of record (tests/shade_env_cases.py).

valid and the route word exact, invalid pixels exactly 0, valid pixels within k FWD_ATOL + FWD_RTOL scale (k = 2 for
reflect_view, K + 2 for shade_env); per-pixel gradients within GRAD_FRAC of their reference's scale
(tests/lighting_cases.py::grad_ratio); parameter gradients within GRAD_FRAC of the sum of their absolute per-pixel
terms (`absum`; tests/test_shade_env_cpu.py holds the framework ops in float32 to half of every bound on the same
cases); every gradient bit-identical from run to run.  Each test prints its worst measured ratios of error to bound.
Measured on an MI355X over all of these tests: shade_env forward at most 0.020 of its bound, per-pixel gradients 0.013,
parameter gradients 0.019; reflect_view 0.046 / 0.006 / 0.015; the chain's gradients at most 0.055.
"""
import ctypes
import functools
import gc
import itertools

import numpy as np
import pytest
import torch

import deferred_cases as dc
import lighting_cases
import shade_env_cases as sec
from dirt_amd import _lib, deferred
from test_shade_env_cpu import REDUCTION_COUNTS, env_measure, reflect_measure

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAMES = sec.PIXEL_NAMES
PARAMS = sec.PARAMS
CHUNK = 256  # the pixels one workgroup of the backwards' first kernel owns


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _node_names(y):
    return [y.grad_fn.name()] + [fn.name() for fn, _ in y.grad_fn.next_functions if fn is not None]


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- shade_env

def _tensors(inputs, L, pix=(True,) * 6, params=PARAMS, dtype=torch.float32):
    """-> (the six per-pixel inputs (occlusion None where inputs[5] is), {parameter name: tensor})"""
    ts = [None if a is None else _gpu(a, dtype).requires_grad_(need) for a, need in zip(inputs, pix)]
    ps = {"coefficients": _gpu(L.coefficients, dtype), "camera": _gpu(L.camera, dtype)}
    for name, p in ps.items():
        p.requires_grad_(name in params)
    return ts, ps


def _call(ts, ps, fn=None):
    return (fn or deferred.shade_env)(ts[0], ts[1], ts[2], ts[3], ps["coefficients"], ts[4], ps["camera"], ts[5])


def _run(inputs, L, grad, pix=(True,) * 6, params=PARAMS, dtype=torch.float32, fn=None):
    """-> dict: pixels, valid (tensors), nodes, grads {name (parameters as 'param_<name>'): numpy, or None where no
    gradient was asked for}"""
    ts, ps = _tensors(inputs, L, pix, params, dtype)
    pixels, valid = _call(ts, ps, fn)
    named = [(n, t) for n, t in zip(NAMES, ts) if t is not None] + [("param_" + n, p) for n, p in ps.items()]
    wrt = [(n, t) for n, t in named if t.requires_grad]
    grads = {n: None for n, _ in named}
    if wrt:
        got = torch.autograd.grad(pixels, [t for _, t in wrt], _gpu(grad, dtype), allow_unused=True)
        for (n, t), g in zip(wrt, got):
            grads[n] = (torch.zeros_like(t) if g is None else g).cpu().numpy()
    torch.cuda.synchronize()
    return {"pixels": pixels.detach(), "valid": valid, "nodes": _node_names(pixels) if wrt else [], "grads": grads}


def _fused(got, name="_ShadeEnvFn"):
    return any(name in n for n in got["nodes"])


def _check(got, L, ref, tag):
    """-> worst ratios (forward, per-pixel gradients, parameter gradients) of error to bound, each at most 1"""
    pixels, valid = got["pixels"].cpu().numpy(), got["valid"].cpu().numpy()
    assert valid.dtype == np.bool_ and valid.shape == ref["valid"].shape + (1,), tag
    v = ref["valid"]
    assert np.array_equal(valid[..., 0], v), tag
    assert np.array_equal(pixels[~v], np.zeros_like(pixels[~v])), tag
    for g in got["grads"].values():
        assert g is None or np.all(np.isfinite(g)), tag
    worst = env_measure((pixels, valid, got["grads"]), L, ref, tag, 1.0)
    print("shade_env %s: forward %.3f of its bound, per-pixel gradients %.3f, parameter gradients %.3f of theirs"
          % ((tag,) + worst))
    return worst


def _same_grads(a, b, tag):
    for name in a["grads"]:
        if a["grads"][name] is None or b["grads"].get(name) is None:
            continue
        assert np.array_equal(_bits(a["grads"][name]), _bits(b["grads"][name])), (tag, name)


def _raw_args(ts, ps, L):
    B, H, W, _ = ts[0].shape
    return (ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), ts[4].data_ptr(),
            None if ts[5] is None else ts[5].data_ptr(), B, H, W, L.K, int(L.coefficients.ndim == 3),
            ps["coefficients"].data_ptr(), int(L.camera.ndim == 2), ps["camera"].data_ptr())


def _raw_fwd(ts, ps, L):
    """dirt_deferred_shade_env_fwd itself -> the route tensor"""
    B, H, W, _ = ts[0].shape
    pixels = torch.empty_like(ts[0])
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    route = torch.empty((B, H, W), dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().dirt_deferred_shade_env_fwd(*_raw_args(ts, ps, L), pixels.data_ptr(), valid.data_ptr(),
                                                       route.data_ptr(), _stream()))
    return route


def _raw_route(inputs, L):
    ts, ps = _tensors(inputs, L, (False,) * 6, ())
    route = _raw_fwd(ts, ps, L)
    torch.cuda.synchronize()
    return route.cpu().numpy().view(np.uint32)


# ---- reflect_view

R_NAMES = ("positions", "normals", "param_camera")


def _rrun(p, n, camera, grad, need=(True,) * 3, dtype=torch.float32, fn=None):
    """-> dict: directions, valid (tensors), nodes, grads {positions, normals, param_camera: numpy or None}"""
    ts = [_gpu(a, dtype).requires_grad_(w) for a, w in zip((p, n, camera), need)]
    directions, valid = (fn or deferred.reflect_view)(*ts)
    wrt = [(k, t) for k, t in zip(R_NAMES, ts) if t.requires_grad]
    grads = {k: None for k in R_NAMES}
    if wrt:
        got = torch.autograd.grad(directions, [t for _, t in wrt], _gpu(grad, dtype), allow_unused=True)
        for (k, t), g in zip(wrt, got):
            grads[k] = (torch.zeros_like(t) if g is None else g).cpu().numpy()
    torch.cuda.synchronize()
    return {"directions": directions.detach(), "valid": valid, "nodes": _node_names(directions) if wrt else [],
            "grads": grads}


def _rcheck(got, ref, tag):
    d, valid = got["directions"].cpu().numpy(), got["valid"].cpu().numpy()
    assert valid.dtype == np.bool_ and valid.shape == ref["valid"].shape + (1,), tag
    v = ref["valid"]
    assert np.array_equal(valid[..., 0], v), tag
    assert np.array_equal(_bits(d[~v]), np.zeros_like(_bits(d[~v]))), tag  # (0, 0, 0) exactly, not -0
    assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=-1)[v] - 1.0) <= 1e-6), tag
    for g in got["grads"].values():
        assert g is None or np.all(np.isfinite(g)), tag
    worst = reflect_measure((d, valid, got["grads"]), ref, tag, 1.0)
    print("reflect_view %s: forward %.3f of its bound, per-pixel gradients %.3f, the camera's %.3f of theirs"
          % ((tag,) + worst))
    return worst


def _rraw(p, n, camera, grad=None, with_camera=True):
    """dirt_deferred_reflect_view_fwd itself -> the route; with grad also dirt_deferred_reflect_view_bwd into
    NaN-filled buffers (the workspace included) -> (route, {name: numpy})"""
    ts = [_gpu(a) for a in (p, n, camera)]
    B, H, W, _ = ts[0].shape
    lib = _lib.load()
    d = torch.empty_like(ts[0])
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    route = torch.empty((B, H, W), dtype=torch.int32, device=DEV)
    pf = int(np.ndim(camera) == 2)
    _lib.check(lib.dirt_deferred_reflect_view_fwd(ts[0].data_ptr(), ts[1].data_ptr(), B, H, W, pf, ts[2].data_ptr(),
                                                  d.data_ptr(), valid.data_ptr(), route.data_ptr(), _stream()))
    out = {}
    if grad is not None:
        out = {"positions": torch.full_like(ts[0], float("nan")), "normals": torch.full_like(ts[1], float("nan"))}
        workspace, size = None, _lib._SZ(0)
        if with_camera:
            out["param_camera"] = torch.full_like(ts[2], float("nan"))
            _lib.check(lib.dirt_deferred_reflect_view_workspace(B, H, W, ctypes.byref(size)))
            assert size.value == B * -(-H * W // CHUNK) * 3 * 4
            workspace = torch.full((size.value // 4,), float("nan"), device=DEV)
        g = _gpu(grad)
        _lib.check(lib.dirt_deferred_reflect_view_bwd(
            ts[0].data_ptr(), ts[1].data_ptr(), B, H, W, pf, ts[2].data_ptr(), g.data_ptr(), route.data_ptr(),
            out["positions"].data_ptr(), out["normals"].data_ptr(),
            out["param_camera"].data_ptr() if with_camera else None,
            None if workspace is None else workspace.data_ptr(), size.value, _stream()))
    torch.cuda.synchronize()
    return route.cpu().numpy().view(np.uint32), {k: t.cpu().numpy() for k, t in out.items()}


# ---- against the statement

@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_matches_the_statement(ident):
    """Both ops over the table of edge frames, every gradient requested, K = 9 with an occlusion."""
    inputs, L, grad, ref = sec.case(ident)
    got = _run(inputs, L, grad)
    assert _fused(got), got["nodes"]
    assert not got["valid"].requires_grad
    assert np.array_equal(_raw_route(inputs, L), ref["route"]), ident
    _check(got, L, ref, ident)
    _same_grads(got, _run(inputs, L, grad), ident)  # bit-identical from run to run
    p, n, camera, g, rref = sec.reflect_case(ident)
    rgot = _rrun(p, n, camera, g)
    assert _fused(rgot, "_ReflectViewFn"), rgot["nodes"]
    assert np.array_equal(_rraw(p, n, camera)[0], rref["route"]), ident
    _rcheck(rgot, rref, ident)
    _same_grads(rgot, _rrun(p, n, camera, g), ident)
    if ident.endswith("all_background"):
        for name, x in list(got["grads"].items()) + list(rgot["grads"].items()):
            assert not np.any(x), (ident, name)  # exactly 0


@pytest.mark.parametrize("count", REDUCTION_COUNTS)
def test_reduction_edges(count):
    """Frames of `count` pixels, and `count` valid pixels in a larger frame: a wave, a workgroup (which is a chunk)
    and four chunks, each one pixel short, full, and one over."""
    for H, W, valid_count in ((1, count, None), (3, 700, count)):
        inputs, L, grad, ref = sec.edge_case(H, W, valid_count=valid_count)
        assert int(ref["valid"].sum()) == count
        tag = "%dx%d with %d valid" % (H, W, count)
        got = _run(inputs, L, grad)
        _check(got, L, ref, tag)
        _same_grads(got, _run(inputs, L, grad), count)
        p, n, camera, g, rref = sec.reflect_of(inputs, L)
        assert int(rref["valid"].sum()) == count
        rgot = _rrun(p, n, camera, g)
        _rcheck(rgot, rref, tag)
        _same_grads(rgot, _rrun(p, n, camera, g), count)


def test_two_frames_of_several_ragged_chunks():
    """33 x 65 = 2145 pixels: nine chunks a frame, the last one ragged, in each of two frames, with shared and with
    per-frame coefficients and cameras."""
    for per_frame in (False, True):
        inputs, L, grad, ref = sec.edge_case(33, 65, B=2, seed=33, per_frame=per_frame, cover=0.7)
        tag = "2x33x65 per_frame=%d" % per_frame
        got = _run(inputs, L, grad)
        _check(got, L, ref, tag)
        _same_grads(got, _run(inputs, L, grad), per_frame)
        p, n, camera, g, rref = sec.reflect_of(inputs, L)
        rgot = _rrun(p, n, camera, g)
        _rcheck(rgot, rref, tag)
        _same_grads(rgot, _rrun(p, n, camera, g), per_frame)


def test_more_chunks_than_the_second_kernel_has_threads():
    """512 x 513: 1026 chunks, four times the reducing workgroup's 256 threads and two over."""
    inputs, L, grad, ref = sec.edge_case(512, 513, seed=512)
    got = _run(inputs, L, grad)
    assert _fused(got)
    _check(got, L, ref, "512x513")
    _same_grads(got, _run(inputs, L, grad), "512x513")
    p, n, camera, g, rref = sec.reflect_of(inputs, L)
    rgot = _rrun(p, n, camera, g)
    _rcheck(rgot, rref, "512x513")
    _same_grads(rgot, _rrun(p, n, camera, g), "512x513")


def _raw_bwd(inputs, L, grad, with_params):
    """dirt_deferred_shade_env_fwd for the route, then dirt_deferred_shade_env_bwd itself into buffers (the workspace
    included) pre-filled with NaN: whatever the launch leaves unwritten stays NaN.  -> {name: numpy}"""
    ts, ps = _tensors(inputs, L, (False,) * 6, ())
    B, H, W, _ = ts[0].shape
    lib = _lib.load()
    route = _raw_fwd(ts, ps, L)
    nan = lambda t: torch.full_like(t, float("nan"))  # noqa: E731
    out = {name: nan(t) for name, t in zip(NAMES, ts) if t is not None}
    workspace, size = None, _lib._SZ(0)
    if with_params:
        out.update({"param_" + name: nan(ps[name]) for name in PARAMS})
        _lib.check(lib.dirt_deferred_shade_env_workspace(B, H, W, L.K, ctypes.byref(size)))
        assert size.value == B * -(-H * W // CHUNK) * (3 + 3 * L.K) * 4
        workspace = torch.full((size.value // 4,), float("nan"), device=DEV)
    ptr = lambda name: out[name].data_ptr() if name in out else None  # noqa: E731
    g = _gpu(grad)
    _lib.check(lib.dirt_deferred_shade_env_bwd(
        *_raw_args(ts, ps, L), g.data_ptr(), route.data_ptr(), ptr("positions"), ptr("colors"), ptr("normals"),
        ptr("material"), ptr("radiance"), ptr("occlusion"), ptr("param_coefficients"), ptr("param_camera"),
        None if workspace is None else workspace.data_ptr(), size.value, _stream()))
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


MANY_FRAMES = 65537  # two more than a grid's second dimension holds


@functools.lru_cache(maxsize=None)
def _many_frames_case(per_frame):
    """65,537 frames of 1 x 2 pixels, every seventh with one background pixel; the cotangents are nonzero in the
    frames of S alone (both ends, the two sides of the grid's 65,535, the middle, five drawn ones).  The frames are
    independent: the statements are evaluated on the frames of S, with the per-frame parameters sliced to them.  A
    frame whose cotangent is zero adds exact zeros to a shared parameter's gradient, so the statement's sums over S
    are the sums over the batch."""
    B = MANY_FRAMES
    rng = np.random.default_rng([65537, int(per_frame)])
    S = np.array(sorted({0, 1, 32767, 65534, 65535, 65536} | set(rng.choice(B, 5, replace=False).tolist())))
    covered = np.ones((B, 1, 2), bool)
    covered[::7, 0, 1] = False
    assert (~covered[S]).any() and covered[S].all(-1).any()
    L = sec.draw_env(rng, B, 9, per_frame)
    LS = L.pick(S) if per_frame else L
    inputs = [a.copy() for a in sec.random_input(rng, covered)]
    settled = sec.settle(rng, tuple(a[S] for a in inputs), LS)
    for a, s in zip(inputs, settled):
        a[S] = s
    grad = np.zeros(inputs[0].shape, np.float32)
    grad[S] = rng.standard_normal(grad[S].shape).astype(np.float32)
    ref = sec.shade_env(*settled, LS, grad[S])
    assert (ref["valid"] & ~covered[S]).any()  # (background pixels that the dilation fills: routes other than own)
    rgrad = np.zeros(inputs[0].shape, np.float32)
    rgrad[S] = rng.standard_normal(grad[S].shape).astype(np.float32)
    rref = sec.reflect_view(settled[0], settled[2], LS.camera, rgrad[S])
    return tuple(inputs), L, grad, S, ref, rgrad, rref


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
def test_more_frames_than_a_grids_y_extent(per_frame):
    """The backwards' first kernels walk `for (frame = blockIdx.y; frame < B; frame += gridDim.y)` under a grid of
    min(B, 65535) rows: at 65,537 frames the workgroups of rows 0 and 1 iterate twice, re-using their LDS sums.  With
    parameter gradients (the kParams kernel and the reduction) and without, through autograd and through the entry
    points themselves into NaN-filled buffers: forward, route and every gradient on the frames of S against the
    statement, exact zeros in every other frame, bit-identical from run to run."""
    inputs, L, grad, S, ref, rgrad, rref = _many_frames_case(per_frame)
    B = MANY_FRAMES
    others = np.ones(B, bool)
    others[S] = False
    at = torch.from_numpy(S).to(DEV)
    tag = "%d frames, %s parameters" % (B, "per-frame" if per_frame else "shared")

    def on_S(grads, out, valid, framed, key):
        for name in framed:
            if grads.get(name) is not None:
                assert grads[name].shape[0] == B and not np.any(grads[name][others]), (tag, name)  # exactly 0
        return {key: out[at], "valid": valid[at],
                "grads": {k: (g[S] if k in framed and g is not None else g) for k, g in grads.items()}}

    framed = NAMES + (("param_coefficients", "param_camera") if per_frame else ())
    LS = L.pick(S) if per_frame else L
    assert np.array_equal(_raw_route(inputs, L)[S], ref["route"])
    full = _run(inputs, L, grad)
    assert _fused(full)
    _check(on_S(full["grads"], full["pixels"], full["valid"], framed, "pixels"), LS, ref, tag + ", all gradients")
    plain = _run(inputs, L, grad, params=())
    _check(on_S(plain["grads"], plain["pixels"], plain["valid"], framed, "pixels"), LS, ref, tag + ", per-pixel alone")
    _same_grads(full, plain, tag)
    for with_params in (True, False):
        raw = _raw_bwd(inputs, L, grad, with_params)
        assert all(np.all(np.isfinite(g)) for g in raw.values()), tag  # nothing was left as it was
        _check(on_S(raw, full["pixels"], full["valid"], framed, "pixels"), LS, ref,
               tag + ", raw, params=%d" % with_params)
        _same_grads(full, {"grads": raw}, tag)
    # reflect_view
    p, n, camera = inputs[0], inputs[2], L.camera
    rframed = ("positions", "normals") + (("param_camera",) if per_frame else ())
    rfull = _rrun(p, n, camera, rgrad)
    assert _fused(rfull, "_ReflectViewFn")
    _rcheck(on_S(rfull["grads"], rfull["directions"], rfull["valid"], rframed, "directions"), rref, tag)
    rplain = _rrun(p, n, camera, rgrad, need=(True, True, False))
    _same_grads(rfull, rplain, tag)
    for with_camera in (True, False):
        route, raw = _rraw(p, n, camera, rgrad, with_camera)
        assert np.array_equal(route[S], rref["route"])
        assert all(np.all(np.isfinite(g)) for g in raw.values()), tag
        _rcheck(on_S(raw, rfull["directions"], rfull["valid"], rframed, "directions"), rref,
                tag + ", raw, camera=%d" % with_camera)
        _same_grads(rfull, {"grads": raw}, tag)


def test_per_frame_parameters_do_not_leak_across_frames():
    """3x5x6-leak with one set of coefficients and one camera per frame: the all-background outer frames' parameter
    gradients are exactly 0, the middle frame's match the statement."""
    inputs, L, grad, ref = sec.case("3x5x6-leak", 9, True)
    got = _run(inputs, L, grad)
    _check(got, L, ref, "leak, per frame")
    for name in PARAMS:
        g = got["grads"]["param_" + name]
        assert g.shape[0] == 3 and not np.any(g[[0, 2]]) and np.any(g[1]), name
    _same_grads(got, _run(inputs, L, grad), "leak")
    p, n, camera, g, rref = sec.reflect_case("3x5x6-leak", True)
    rgot = _rrun(p, n, camera, g)
    _rcheck(rgot, rref, "leak, per frame")
    gc_ = rgot["grads"]["param_camera"]
    assert gc_.shape == (3, 3) and not np.any(gc_[[0, 2]]) and np.any(gc_[1])


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
@pytest.mark.parametrize("K", sec.COUNTS)
def test_coefficient_counts(K, per_frame):
    ident = "3x5x6-leak" if per_frame else "15x17-checkerboard"
    inputs, L, grad, ref = sec.case(ident, K, per_frame)
    got = _run(inputs, L, grad)
    assert _fused(got) and got["grads"]["param_coefficients"].shape == L.coefficients.shape
    _check(got, L, ref, "K=%d per_frame=%d" % (K, per_frame))
    _same_grads(got, _run(inputs, L, grad), K)


def test_no_occlusion_is_an_occlusion_of_ones():
    """occlusion=None against ones: the same bits in pixels and gradients, against the statement too."""
    inputs, L, grad, ref = sec.case("15x17-island", 9, False, False)
    ones = inputs[:5] + (np.ones(inputs[0].shape[:-1] + (1,), np.float32),)
    a, b = _run(ones, L, grad), _run(inputs, L, grad)
    assert _fused(a) and _fused(b) and torch.equal(a["pixels"], b["pixels"]) and "occlusion" not in b["grads"]
    _same_grads(a, b, "no occlusion")
    _check(b, L, ref, "no occlusion")
    _check(a, L, sec.shade_env(*ones, L, grad), "occlusion of ones")


def test_clamp_ends():
    """The material exactly on and past the clamps' ends: within the bounds, the closed-interval derivative nonzero at
    the ends, exactly 0 at a roughness below R_MIN and past every end."""
    inputs, L, grad, ref = sec.clamp_ends_case()
    got = _run(inputs, L, grad)
    _check(got, L, ref, "clamp ends")
    g, v = got["grads"]["material"], ref["valid"]
    rough, metal = inputs[3][..., 0], inputs[3][..., 1]
    assert np.all(g[..., 0][(rough == 0.0) | (rough == 1.5)] == 0)
    assert np.all(g[..., 1][(metal == -0.5) | (metal == 1.5)] == 0)
    for on in (rough == np.float32(0.045), rough == 1.0):
        assert np.abs(g[..., 0][on & v]).min() > 0
    for on in (metal == 0.0, metal == 1.0):
        assert np.abs(g[..., 1][on & v]).min() > 0


def test_gradient_subsets(monkeypatch):
    """Every gradient requested alone, every subset of the per-pixel inputs with all and with no parameter, every
    subset of the parameters with all the per-pixel inputs: the requested gradients are bit-identical to the
    all-requested run's, the others None; the per-pixel gradients do not depend on whether a parameter is requested
    (one kernel with the sums, one without).  With no parameter gradient requested no workspace is asked for."""
    lib = _lib.load()
    asked = []
    for op in ("shade_env", "reflect_view"):
        real = getattr(lib, "dirt_deferred_%s_workspace" % op)
        monkeypatch.setattr(lib, "dirt_deferred_%s_workspace" % op,
                            lambda *a, real=real, op=op: (asked.append(op), real(*a))[1])
    inputs, L, grad, ref = sec.case("15x17-block_br")
    full = _run(inputs, L, grad)
    assert asked == ["shade_env"]
    _check(full, L, ref, "all gradients")
    none = (False,) * 6
    subsets = [(tuple(i == j for i in range(6)), ()) for j in range(6)] + [(none, (name,)) for name in PARAMS]
    subsets += [(g, p) for g in itertools.product((False, True), repeat=6) for p in ((), PARAMS)]
    subsets += [((True,) * 6, (name,)) for name in PARAMS]
    for pix, params in subsets:
        del asked[:]
        got = _run(inputs, L, grad, pix, params)
        assert asked == (["shade_env"] if params else []), (pix, params)
        assert torch.equal(got["pixels"], full["pixels"])
        for name, need in list(zip(NAMES, pix)) + [("param_" + n, n in params) for n in PARAMS]:
            assert (got["grads"][name] is not None) == need, (pix, params, name)
        _same_grads(got, full, (pix, params))
        if any(pix) or params:
            assert _fused(got)
    p, n, camera, g, rref = sec.reflect_case("15x17-block_br")
    del asked[:]
    rfull = _rrun(p, n, camera, g)
    assert asked == ["reflect_view"]
    for need in itertools.product((False, True), repeat=3):
        del asked[:]
        rgot = _rrun(p, n, camera, g, need)
        assert asked == (["reflect_view"] if need[2] else []), need
        assert torch.equal(rgot["directions"], rfull["directions"])
        for name, w in zip(R_NAMES, need):
            assert (rgot["grads"][name] is not None) == w, (need, name)
        _same_grads(rgot, rfull, need)


def test_nan_normal_invalidates_only_its_reach():
    """A NaN normal at a covered pixel on the silhouette: that pixel and the background neighbours whose window holds
    it are invalid; every output and gradient, the parameters' included, stays finite and as the statement's."""
    ident = "15x17-block_tl"  # covered rows 0..7, columns 0..8
    clean, L, grad, _ = sec.case(ident)
    inputs = tuple(a.copy() for a in clean)
    inputs[2][0, 7, 8, 1] = np.nan
    ref = sec.shade_env(*inputs, L, grad)
    for y, x0 in ((7, 8), (8, 7), (8, 8), (8, 9), (7, 9), (6, 9)):
        assert not ref["valid"][0, y, x0]
    assert ref["valid"][0, 6, 8] and ref["valid"][0, 5, 9]
    got = _run(inputs, L, grad)
    _check(got, L, ref, "nan normal")
    assert bool(torch.isfinite(got["pixels"]).all())
    p, n, camera, g, _ = sec.reflect_case(ident)
    rref = sec.reflect_view(p, inputs[2], camera, g)
    assert np.array_equal(rref["valid"], ref["valid"])
    rgot = _rrun(p, inputs[2], camera, g)
    _rcheck(rgot, rref, "nan normal")
    assert bool(torch.isfinite(rgot["directions"]).all())


@pytest.mark.parametrize("which", ["material", "radiance", "occlusion"])
def test_nan_in_an_undilated_input_stays_at_its_pixel(which):
    """A NaN roughness, radiance or occlusion at an interior pixel: NaN at that pixel and nowhere else (they are read
    undilated, like the colour); a NaN on the background, out of every window's reach, is never read."""
    ident = "15x17-block_tl"
    clean, L, grad, ref = sec.case(ident)
    i = NAMES.index(which)
    dirty = tuple(a.copy() for a in clean)
    y, x0 = 3, 4
    dirty[i][0, y, x0, 0] = np.nan
    dirty[i][0, 12, 12, 0] = np.nan  # background, out of every window's reach: invalid, never read
    got = _run(dirty, L, grad, params=())
    pixels = got["pixels"].cpu().numpy()
    nan = np.isnan(pixels).any(-1)
    assert nan[0, y, x0] and nan.sum() == 1
    keep = ~nan
    assert np.array_equal(_bits(pixels[keep]), _bits(_run(clean, L, grad, params=())["pixels"].cpu().numpy()[keep]))
    for name in ("colors", "material", "radiance", "occlusion"):
        assert np.all(np.isfinite(got["grads"][name][keep])), name
    for name in ("positions", "normals"):  # the pixel's own adjoint reaches its 3 x 3 neighbourhood at most
        far = np.ones(nan.shape, bool)
        far[0, y - 1:y + 2, x0 - 1:x0 + 2] = False
        assert np.all(np.isfinite(got["grads"][name][far])), name


def test_forms(monkeypatch):
    """[H,W,.] and non-contiguous inputs run the fused kernels and give the batched, contiguous result; float64,
    DIRT_FUSED_DEFERRED=0 and CPU tensors take the statements."""
    inputs, L, grad, ref = sec.case("15x17-island")
    base = _run(inputs, L, grad)
    one = _run([a[0] for a in inputs], L, grad[0])
    assert one["pixels"].shape == (15, 17, 3) and one["valid"].shape == (15, 17, 1) and _fused(one)
    assert torch.equal(one["pixels"], base["pixels"][0])
    for name in base["grads"]:
        assert np.array_equal(_bits(one["grads"][name]).reshape(-1), _bits(base["grads"][name]).reshape(-1)), name
    wide = [torch.zeros(a.shape[:-1] + (2 * a.shape[-1],), device=DEV) for a in inputs]
    for w, a in zip(wide, inputs):
        w[..., ::2] = _gpu(a)
    ts, ps = _tensors(inputs, L)
    wide_coef = torch.zeros((9, 6), device=DEV)
    wide_coef[:, ::2] = ps["coefficients"].detach()
    wc = wide_coef.requires_grad_(True)
    ws = [w.requires_grad_(True) for w in wide]
    pixels, valid = _call([w[..., ::2] for w in ws], dict(ps, coefficients=wc[:, ::2]))
    assert any("_ShadeEnvFn" in x for x in _node_names(pixels))
    pixels.backward(_gpu(grad))
    assert torch.equal(pixels.detach(), base["pixels"]) and torch.equal(valid, base["valid"])
    for w, name in zip(ws, NAMES):
        assert np.array_equal(_bits(w.grad.cpu().numpy()[..., ::2]), _bits(base["grads"][name])), name
    assert np.array_equal(_bits(wc.grad.cpu().numpy()[:, ::2]), _bits(base["grads"]["param_coefficients"]))
    p, n, camera, g, rref = sec.reflect_case("15x17-island")
    rbase = _rrun(p, n, camera, g)
    rone = _rrun(p[0], n[0], camera, g[0])
    assert rone["directions"].shape == (15, 17, 3) and _fused(rone, "_ReflectViewFn")
    assert torch.equal(rone["directions"], rbase["directions"][0])
    for name in R_NAMES:
        assert np.array_equal(_bits(rone["grads"][name]).reshape(-1), _bits(rbase["grads"][name]).reshape(-1)), name
    wp, wn = (torch.zeros(p.shape[:-1] + (6,), device=DEV) for _ in range(2))
    wp[..., ::2], wn[..., ::2] = _gpu(p), _gpu(n)
    d, _ = deferred.reflect_view(wp[..., ::2], wn[..., ::2], _gpu(camera))
    assert torch.equal(d, rbase["directions"])

    def statement(got, tol_fwd):
        assert not _fused(got), got["nodes"]
        assert np.array_equal(got["valid"].cpu().numpy()[..., 0], ref["valid"])
        assert np.all(np.abs(got["pixels"].cpu().numpy() - ref["pixels"]) <= tol_fwd)

    f64 = _run(inputs, L, grad, dtype=torch.float64)
    statement(f64, 1e-12)
    for name, want in ref["params"].items():
        got = f64["grads"]["param_" + name].reshape(np.shape(want))
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    r64 = _rrun(p, n, camera, g, dtype=torch.float64)
    assert not _fused(r64, "_ReflectViewFn")
    assert np.abs(r64["directions"].cpu().numpy() - rref["directions"]).max() <= 1e-12
    assert np.abs(r64["grads"]["param_camera"] - rref["params"]["camera"]).max() <= 1e-12
    cpu = deferred.shade_env(*[torch.from_numpy(a) for a in inputs[:4]],
                             torch.from_numpy(L.coefficients).requires_grad_(True), torch.from_numpy(inputs[4]),
                             torch.from_numpy(L.camera).requires_grad_(True), torch.from_numpy(inputs[5]))
    assert "_ShadeEnvFn" not in cpu[0].grad_fn.name() and cpu[0].device.type == "cpu"
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    statement(_run(inputs, L, grad), sec.fwd_bound(ref, L.K))
    assert not _fused(_rrun(p, n, camera, g), "_ReflectViewFn")


def test_double_backward_raises_on_the_fused_path():
    inputs, L, grad, ref = sec.case("15x17-hole")
    ts, ps = _tensors(inputs, L)
    pixels, _ = _call(ts, ps)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(pixels.square().sum(), [ps["coefficients"]], create_graph=True)
    directions, _ = deferred.reflect_view(ts[0], ts[2], ps["camera"])
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(directions.square().sum(), [ps["camera"]], create_graph=True)


def _chain_of(ts, ps, cubemap):
    """the three-op chain the two ops were added for"""
    chain = deferred.build_cubemap_mipmaps(cubemap)
    directions, _ = deferred.reflect_view(ts[0], ts[2], ps["camera"])
    radiance, _ = deferred.sample_cubemap_mip(chain, directions, lod=ts[3][..., 0] * (len(chain) - 1))
    return deferred.shade_env(ts[0], ts[1], ts[2], ts[3], ps["coefficients"], radiance, ps["camera"], occlusion=ts[5])


def test_captures_into_a_graph():
    """One forward and backward of both ops with every gradient captured with torch.cuda.graph, replayed after every
    input changed in place: equal to the eager result bit for bit."""
    first, L1, grad, _ = sec.case("63x65-block_tl")
    second, L2, _, _ = sec.case("63x65-checkerboard")
    ts, ps = _tensors(first, L1)
    g = _gpu(grad)
    named = list(zip(NAMES, ts)) + [("param_" + n, p) for n, p in ps.items()]
    rwrt = [ts[0], ts[2], ps["camera"]]
    out = {}

    def step():
        pixels, valid = _call(ts, ps)
        out["pixels"], out["valid"] = pixels, valid
        out["grads"] = torch.autograd.grad(pixels, [t for _, t in named], g)
        directions, _ = deferred.reflect_view(*rwrt)
        out["directions"] = directions
        out["rgrads"] = torch.autograd.grad(directions, rwrt, g)

    gc.collect()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    with torch.no_grad():
        for t, a in zip(ts, second):
            t.copy_(_gpu(a))
        for name in PARAMS:
            ps[name].copy_(_gpu(getattr(L2, name)))
    graph.replay()
    torch.cuda.synchronize()
    got = (out["pixels"].detach().clone(), out["valid"].clone(), [x.clone() for x in out["grads"]],
           out["directions"].detach().clone(), [x.clone() for x in out["rgrads"]])
    del graph
    out.clear()
    eager = _run(second, L2, grad)
    assert torch.equal(got[0], eager["pixels"]) and torch.equal(got[1], eager["valid"])
    for (name, _), a in zip(named, got[2]):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(eager["grads"][name])), name
    reager = _rrun(second[0], second[2], L2.camera, grad)
    assert torch.equal(got[3], reager["directions"])
    for name, a in zip(R_NAMES, got[4]):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(reager["grads"][name])), name


# ---- the chain

def _chain(H=64, W=64, S=16):
    """reflect_view -> sample_cubemap_mip over an S x S chain at lod = roughness (levels - 1) -> shade_env on a frame
    with a covered disc -> sum(pixels * weights), and its gradients to the cube map, the coefficients, the material,
    the normals, the positions and the camera"""
    rng = np.random.default_rng(64)
    yy, xx = np.mgrid[0:H, 0:W]
    covered = (((yy - H / 2 + 0.5) ** 2 + (xx - W / 2 + 0.5) ** 2) < (0.4 * H) ** 2)[None]
    L = sec.draw_env(rng, 1)
    # (roughness in [0.06, 0.97]: the lod stays inside the chain's levels)
    inputs = sec.settle(rng, sec.random_input(rng, covered, roughness=(0.06, 0.97)), L)
    cube = rng.uniform(0.2, 2.0, (6, S, S, 3)).astype(np.float32)
    wts = rng.uniform(0.0, 1.0, inputs[0].shape).astype(np.float32)
    ts, ps = _tensors(inputs, L)
    cubemap = _gpu(cube).requires_grad_(True)
    pixels, valid = _chain_of(ts, ps, cubemap)
    loss = (pixels * _gpu(wts)).sum()
    wrt = {"cubemap": cubemap, "coefficients": ps["coefficients"], "material": ts[3], "normals": ts[2],
           "positions": ts[0], "camera": ps["camera"]}
    grads = torch.autograd.grad(loss, list(wrt.values()))
    return dict(pixels=pixels.detach(), valid=valid, pixel_node=pixels,
                grads={k: g.cpu().numpy() for k, g in zip(wrt, grads)})


def test_chain_reflection_cube_lookup_and_environment(monkeypatch):
    """The image-based-lighting chain at 64 x 64 over an S = 16 cube chain (`_chain`): the fused ops against the same
    chain with every op on the framework path (DIRT_FUSED_DEFERRED=0) on the GPU.  valid equal, and no mask anywhere:
    the unreached background is left out by the zero direction.  Every gradient -- cube map, coefficients, roughness /
    metallic map, normals, positions, camera -- within GRAD_FRAC of its scale (lighting_cases.grad_ratio); the pixels,
    at most about 10 in magnitude here, within FWD_RTOL of that, 1e-4."""
    fused = _chain()
    assert any("_ShadeEnvFn" in x for x in _node_names(fused["pixel_node"]))
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    ops = _chain()
    assert not any("_ShadeEnvFn" in x for x in _node_names(ops["pixel_node"]))
    assert torch.equal(fused["valid"], ops["valid"]) and bool(fused["valid"].any()) and not bool(fused["valid"].all())
    assert not bool(fused["pixels"][~fused["valid"][..., 0]].any())
    ratios = {k: lighting_cases.grad_ratio(fused["grads"][k], ops["grads"][k], k) for k in fused["grads"]}
    px = float((fused["pixels"] - ops["pixels"]).abs().max())
    print("env chain 64x64: pixels differ by at most %.3g; gradient ratios %s"
          % (px, {k: round(v, 4) for k, v in ratios.items()}))
    assert all(np.abs(g).max() > 0 for g in fused["grads"].values())
    assert px <= 1e-4 and all(r <= 1.0 for r in ratios.values()), ratios
