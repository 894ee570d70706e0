"""The fused shade_pbr kernels (dirt_amd/csrc/shade_pbr_kernels.h through dirt_amd.deferred.shade_pbr) against the
float64 statement of record (tests/shade_pbr_cases.py).

valid and the route word exact, invalid pixels exactly 0, valid pixels within (1 + 2 N) * FWD_ATOL + FWD_RTOL * scale;
per-pixel gradients (positions, colors, normals, material, visibility) within GRAD_FRAC of their reference's scale
(tests/lighting_cases.py::grad_ratio); parameter gradients within GRAD_FRAC of the sum of their absolute per-pixel
terms (`absum`; tests/test_shade_pbr_cpu.py holds the framework ops in float32 to half of every bound on the same
cases), frames with a single valid pixel left out of that one check; every gradient bit-identical from run to run.
Each test prints its worst measured ratios of error to bound.
"""
import ctypes
import functools
import gc
import itertools

import numpy as np
import pytest
import torch

import deferred_cases as dc
import deferred_pipeline as dp
import lighting_cases
import shade_pbr_cases as spc
from dirt_amd import _lib, deferred
from test_shade_pbr_cpu import LOW_ROUGHNESS_W, low_roughness_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAMES = spc.PIXEL_NAMES
PARAMS = spc.PARAMS
FRAC = lighting_cases.GRAD_FRAC
CHUNK = 256  # the pixels one workgroup of the backward's first kernel owns


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _node_names(y):
    return [y.grad_fn.name()] + [fn.name() for fn, _ in y.grad_fn.next_functions if fn is not None]


def _tensors(inputs, L, pix=(True,) * 5, params=PARAMS, dtype=torch.float32):
    """-> (the five per-pixel inputs (visibility None where inputs[4] is), {parameter name: tensor})"""
    ts = [None if a is None else _gpu(a, dtype).requires_grad_(need) for a, need in zip(inputs, pix)]
    ps = {"vectors": _gpu(L.vectors, dtype), "colors": _gpu(L.colors, dtype), "camera": _gpu(L.camera, dtype)}
    if L.ambient is not None:
        ps["ambient"] = _gpu(L.ambient, dtype)
    for name, p in ps.items():
        p.requires_grad_(name in params)
    return ts, ps


def _call(ts, ps, L, fn=None):
    return (fn or deferred.shade_pbr)(ts[0], ts[1], ts[2], ts[3], ps["vectors"], ps["colors"], ps["camera"],
                                      ps.get("ambient"), L.point, ts[4])


def _run(inputs, L, grad, pix=(True,) * 5, params=PARAMS, dtype=torch.float32, fn=None):
    """-> dict: pixels, valid (tensors), nodes, grads {name (parameters as 'param_<name>'): numpy, or None where no
    gradient was asked for}"""
    ts, ps = _tensors(inputs, L, pix, params, dtype)
    pixels, valid = _call(ts, ps, L, fn)
    named = [(n, t) for n, t in zip(NAMES, ts) if t is not None] + [("param_" + n, p) for n, p in ps.items()]
    wrt = [(n, t) for n, t in named if t.requires_grad]
    grads = {n: None for n, _ in named}
    if wrt:
        got = torch.autograd.grad(pixels, [t for _, t in wrt], _gpu(grad, dtype), allow_unused=True)
        for (n, t), g in zip(wrt, got):
            grads[n] = (torch.zeros_like(t) if g is None else g).cpu().numpy()
    torch.cuda.synchronize()
    return {"pixels": pixels.detach(), "valid": valid, "nodes": _node_names(pixels) if wrt else [], "grads": grads}


def _fused(got):
    return any("_ShadePbrFn" in n for n in got["nodes"])


def _check(got, ref, n, tag, accuracy=True, fwd_limit=1.0):
    """-> worst ratios (forward, per-pixel gradients, parameter gradients) of error to bound"""
    pixels, valid = got["pixels"].cpu().numpy(), got["valid"].cpu().numpy()
    assert valid.dtype == np.bool_ and valid.shape == ref["valid"].shape + (1,), tag
    assert np.array_equal(valid[..., 0], ref["valid"]), tag
    v = ref["valid"]
    assert np.array_equal(pixels[~v], np.zeros_like(pixels[~v])), tag
    err, bound = np.abs(pixels - ref["pixels"])[v], spc.fwd_bound(ref, n)[v]
    fwd = float((err / bound).max()) if err.size else 0.0
    worst_g = worst_p = 0.0
    for name in NAMES:
        if got["grads"].get(name) is not None and got["grads"][name].size:  # (N = 0: an empty visibility)
            r = lighting_cases.grad_ratio(got["grads"][name], ref[name], "%s d %s" % (tag, name))
            assert r <= 1.0, (tag, name, r)
            worst_g = max(worst_g, r)
    for name, want in ref["params"].items():
        g = got["grads"].get("param_" + name)
        if g is None or np.size(want) == 0:
            continue
        assert np.all(np.isfinite(g)), (tag, name)
        if accuracy:
            r = spc.param_ratio(g, want, ref["absum"][name], FRAC)
            assert r <= 1.0, (tag, name, r)
            worst_p = max(worst_p, r)
    print("shade_pbr %s: forward %.3f of its bound, per-pixel gradients %.3f, parameter gradients %.3f of theirs"
          % (tag, fwd, worst_g, worst_p))
    assert fwd <= fwd_limit, (tag, fwd)
    return fwd, worst_g, worst_p


def _same_grads(a, b, tag):
    for name in a["grads"]:
        if a["grads"][name] is None or b["grads"].get(name) is None:
            continue
        assert np.array_equal(_bits(a["grads"][name]), _bits(b["grads"][name])), (tag, name)


def _raw_args(ts, ps, L):
    B, H, W, _ = ts[0].shape
    amb = ps.get("ambient")
    return (ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(),
            None if ts[4] is None or L.n == 0 else ts[4].data_ptr(), B, H, W, None if amb is None else amb.data_ptr(),
            L.n, sum(1 << i for i, on in enumerate(L.point) if on), int(L.vectors.ndim == 3), ps["vectors"].data_ptr(),
            ps["colors"].data_ptr(), int(L.camera.ndim == 2), ps["camera"].data_ptr())


def _raw_fwd(ts, ps, L):
    """dirt_deferred_shade_pbr_fwd itself -> the route tensor"""
    B, H, W, _ = ts[0].shape
    pixels = torch.empty_like(ts[0])
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    route = torch.empty((B, H, W), dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().dirt_deferred_shade_pbr_fwd(*_raw_args(ts, ps, L), pixels.data_ptr(), valid.data_ptr(),
                                                       route.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream))
    return route


def _raw_route(inputs, L):
    ts, ps = _tensors(inputs, L, (False,) * 5, ())
    route = _raw_fwd(ts, ps, L)
    torch.cuda.synchronize()
    return route.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_matches_the_statement(ident):
    """One directional and one point light over the table of edge frames, every gradient requested.  Measured on an
    MI355X over the table: forward at most 0.562 of its bound (63x65-block_br), per-pixel gradients 0.074, parameter
    gradients 0.040."""
    inputs, L, grad, ref = spc.case(ident)
    got = _run(inputs, L, grad)
    assert _fused(got), got["nodes"]
    assert not got["valid"].requires_grad
    assert np.array_equal(_raw_route(inputs, L), ref["route"]), ident
    _check(got, ref, L.n, ident, accuracy=ident in spc.accuracy_frames())
    _same_grads(got, _run(inputs, L, grad), ident)  # bit-identical from run to run
    if ident.endswith("all_background"):
        for name, g in got["grads"].items():
            assert not np.any(g), (ident, name)  # exactly 0


def _edge_case(H, W, B=1, valid_count=None, seed=0, n=2, **lights):
    """A fully covered frame (valid_count: only its first pixels have a usable normal)"""
    rng = np.random.default_rng([seed, H, W, B, valid_count or 0])
    covered = np.ones((B, H, W), bool)
    invalid = None
    if valid_count is not None:
        invalid = (np.arange(H * W) >= valid_count).reshape(1, H, W).repeat(B, 0)
    inputs = spc.random_input(rng, covered, n, invalid)
    L = spc.draw_lights(rng, B, n, **lights)
    grad = rng.standard_normal(inputs[0].shape).astype(np.float32)
    return inputs, L, grad


@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_reduction_edges(count):
    """Frames of `count` pixels, and `count` valid pixels in a larger frame: a wave, a workgroup (which is a chunk)
    and four chunks, each one pixel short, full, and one over.  Measured on an MI355X: forward at most 0.203 of its
    bound, per-pixel gradients 0.077, parameter gradients 0.052."""
    for H, W, valid_count in ((1, count, None), (3, 700, count)):
        inputs, L, grad = _edge_case(H, W, valid_count=valid_count)
        ref = spc.shade_pbr(*inputs, L, grad)
        assert int(ref["valid"].sum()) == count
        got = _run(inputs, L, grad)
        _check(got, ref, L.n, "%dx%d with %d valid" % (H, W, count))
        _same_grads(got, _run(inputs, L, grad), count)


def test_two_frames_of_several_ragged_chunks():
    """33 x 65 = 2145 pixels: nine chunks a frame, the last one ragged, in each of two frames, with shared and with
    per-frame lights.  Measured on an MI355X (shared / per-frame): forward 0.113 / 0.066 of its bound, per-pixel
    gradients 0.075 / 0.057, parameter gradients 0.004 / 0.009."""
    rng = np.random.default_rng(33)
    covered = rng.random((2, 33, 65)) < 0.7
    inputs = spc.random_input(rng, covered, 3)
    grad = rng.standard_normal(inputs[0].shape).astype(np.float32)
    for per_frame in (False, True):
        L = spc.draw_lights(rng, 2, 3, "mixed", per_frame)
        ref = spc.shade_pbr(*inputs, L, grad)
        got = _run(inputs, L, grad)
        _check(got, ref, L.n, "2x33x65 per_frame=%d" % per_frame)
        _same_grads(got, _run(inputs, L, grad), per_frame)


def test_more_chunks_than_the_second_kernel_has_threads():
    """512 x 513: 1026 chunks, four times the reducing workgroup's 256 threads and two over.  Against `_shade_pbr_ops`
    in float64 on the GPU; scale and absum (the bounds' scales) from the statement, which is plain numpy here: the
    frame has one background row only.  Measured on an MI355X: forward 0.114 of its bound, per-pixel gradients 0.026,
    parameter gradients 0.001."""
    rng = np.random.default_rng(512)
    covered = np.ones((1, 512, 513), bool)
    covered[0, 300] = False
    inputs = spc.random_input(rng, covered, 2)
    L = spc.draw_lights(rng, 1, 2, "mixed")
    grad = rng.standard_normal(inputs[0].shape).astype(np.float32)
    got = _run(inputs, L, grad)
    assert _fused(got)
    want = _run(inputs, L, grad, dtype=torch.float64, fn=deferred._shade_pbr_ops)
    stmt = spc.shade_pbr(*inputs, L, grad)
    ref = dict(stmt, pixels=want["pixels"].cpu().numpy(),
               params={k: want["grads"]["param_" + k].reshape(np.shape(v)) for k, v in stmt["params"].items()})
    for name in NAMES:
        ref[name] = want["grads"][name]
    assert np.array_equal(want["valid"].cpu().numpy()[..., 0], stmt["valid"])
    _check(got, ref, L.n, "512x513")
    _same_grads(got, _run(inputs, L, grad), "512x513")


def _raw_bwd(inputs, L, grad, with_params):
    """dirt_deferred_shade_pbr_fwd for the route, then dirt_deferred_shade_pbr_bwd itself into buffers (the workspace
    included) pre-filled with NaN: whatever the launch leaves unwritten stays NaN.  -> {name: numpy}"""
    ts, ps = _tensors(inputs, L, (False,) * 5, ())
    B, H, W, _ = ts[0].shape
    lib, stream = _lib.load(), torch.cuda.current_stream(DEV).cuda_stream
    route = _raw_fwd(ts, ps, L)
    nan = lambda t: torch.full_like(t, float("nan"))  # noqa: E731
    out = {name: nan(t) for name, t in zip(NAMES, ts)}
    workspace, size = None, _lib._SZ(0)
    if with_params:
        out.update({"param_" + name: nan(ps[name]) for name in PARAMS})
        _lib.check(lib.dirt_deferred_shade_pbr_workspace(B, H, W, L.n, ctypes.byref(size)))
        assert size.value == B * -(-H * W // CHUNK) * (6 + 6 * L.n) * 4
        workspace = torch.full((size.value // 4,), float("nan"), device=DEV)
    ptr = lambda name: out[name].data_ptr() if name in out else None  # noqa: E731
    g = _gpu(grad)
    _lib.check(lib.dirt_deferred_shade_pbr_bwd(
        *_raw_args(ts, ps, L), g.data_ptr(), route.data_ptr(), ptr("positions"), ptr("colors"), ptr("normals"),
        ptr("material"), ptr("visibility"), ptr("param_ambient"), ptr("param_vectors"), ptr("param_colors"),
        ptr("param_camera"), None if workspace is None else workspace.data_ptr(), size.value, stream))
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


MANY_FRAMES = 65537  # two more than a grid's second dimension holds


@functools.lru_cache(maxsize=None)
def _many_frames_case(per_frame):
    """65,537 frames of 1 x 3 pixels, every seventh with one background pixel; the cotangent is nonzero in the frames
    of S alone (both ends, the two sides of the grid's 65,535, the middle, five drawn ones).  The frames are
    independent: the statement is evaluated on the frames of S, with the per-frame lights sliced to them.  A frame
    whose cotangent is zero adds exact zeros to a shared parameter's gradient, so the statement's sums over S are the
    sums over the batch."""
    B = MANY_FRAMES
    rng = np.random.default_rng([65537, int(per_frame)])
    S = np.array(sorted({0, 1, 32767, 65534, 65535, 65536} | set(rng.choice(B, 5, replace=False).tolist())))
    covered = np.ones((B, 1, 3), bool)
    covered[::7, 0, 1] = False
    assert (~covered[S]).any() and covered[S].all(-1).any()
    inputs = spc.random_input(rng, covered, 2)
    L = spc.draw_lights(rng, B, 2, "mixed", per_frame)
    grad = np.zeros(inputs[0].shape, np.float32)
    grad[S] = rng.standard_normal(grad[S].shape).astype(np.float32)
    pick = (lambda a: a[S]) if per_frame else (lambda a: a)
    LS = spc.LightSet(pick(L.vectors), pick(L.colors), pick(L.camera), L.ambient, L.point)
    ref = spc.shade_pbr(*[a[S] for a in inputs], LS, grad[S])
    assert (ref["valid"] & ~covered[S]).any()  # (background pixels that the dilation fills: routes other than own)
    return inputs, L, grad, S, ref


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
def test_more_frames_than_a_grids_y_extent(per_frame):
    """The backward's first kernel walks `for (frame = blockIdx.y; frame < B; frame += gridDim.y)` under a grid of
    min(B, 65535) rows: at 65,537 frames the workgroups of rows 0 and 1 iterate twice, re-using their LDS sums.  With
    parameter gradients (the kParams kernel and the reduction) and without, through autograd and through the entry
    point itself into NaN-filled buffers: forward, route and every gradient on the frames of S against the statement,
    exact zeros in every other frame, bit-identical from run to run.  Measured on an MI355X: forward at most 0.003 of
    its bound, per-pixel gradients 0.041, parameter gradients 0.073."""
    inputs, L, grad, S, ref = _many_frames_case(per_frame)
    B = MANY_FRAMES
    others = np.ones(B, bool)
    others[S] = False
    framed = NAMES + (("param_vectors", "param_colors", "param_camera") if per_frame else ())
    assert np.array_equal(_raw_route(inputs, L)[S], ref["route"])
    tag = "%d frames, %s lights" % (B, "per-frame" if per_frame else "shared")

    def on_S(grads, pixels, valid):
        for name in framed:
            if grads.get(name) is not None:
                assert grads[name].shape[0] == B and not np.any(grads[name][others]), (tag, name)  # exactly 0
        at = torch.from_numpy(S).to(DEV)
        return {"pixels": pixels[at], "valid": valid[at],
                "grads": {k: (g[S] if k in framed and g is not None else g) for k, g in grads.items()}}

    full = _run(inputs, L, grad)
    assert _fused(full)
    _check(on_S(full["grads"], full["pixels"], full["valid"]), ref, L.n, tag + ", all gradients")
    plain = _run(inputs, L, grad, params=())
    _check(on_S(plain["grads"], plain["pixels"], plain["valid"]), ref, L.n, tag + ", per-pixel alone")
    _same_grads(full, plain, tag)
    for with_params in (True, False):
        raw = _raw_bwd(inputs, L, grad, with_params)
        assert all(np.all(np.isfinite(g)) for g in raw.values()), tag  # nothing was left as it was
        _check(on_S(raw, full["pixels"], full["valid"]), ref, L.n, tag + ", raw, params=%d" % with_params)
        _same_grads(full, {"grads": raw}, tag)


def test_per_frame_lights_do_not_leak_across_frames():
    """3x5x6-leak with one set of lights and one camera per frame: the all-background outer frames' parameter gradients
    are exactly 0, the middle frame's match the statement."""
    inputs, L, grad, ref = spc.case("3x5x6-leak", 2, "mixed", True)
    got = _run(inputs, L, grad)
    _check(got, ref, L.n, "leak, per frame")
    for name in ("vectors", "colors", "camera"):
        g = got["grads"]["param_" + name]
        assert g.shape[0] == 3 and not np.any(g[[0, 2]]) and np.any(g[1]), name
    _same_grads(got, _run(inputs, L, grad), "leak")


@pytest.mark.parametrize("kinds", ["directional", "point", "mixed"])
@pytest.mark.parametrize("n", [0, 1, 8])
def test_light_counts_and_kinds(n, kinds):
    """Measured on an MI355X: forward at most 0.106 of its bound, per-pixel gradients 0.069, parameter gradients 0.070
    (all three at N = 8 directional)."""
    inputs, L, grad, ref = spc.case("15x17-checkerboard", n, kinds)
    got = _run(inputs, L, grad)
    assert _fused(got)
    _check(got, ref, n, "N=%d %s" % (n, kinds))
    if n == 0:
        assert not np.any(got["grads"]["param_camera"])
        assert got["grads"]["param_vectors"].shape == (0, 3)


def test_visibility():
    """visibility=None against ones: the same bits in pixels and gradients.  A visibility of zeros on one light removes
    that light exactly, while its visibility gradient still is the statement's."""
    inputs, L, grad, _ = spc.case("15x17-checkerboard", 3, "mixed")
    ones = inputs[:4] + (np.ones_like(inputs[4]),)
    a, b = _run(ones, L, grad), _run(inputs[:4] + (None,), L, grad)
    assert _fused(a) and _fused(b) and torch.equal(a["pixels"], b["pixels"]) and b["grads"].get("visibility") is None
    _same_grads(a, b, "no visibility")
    off = inputs[4].copy()
    off[..., 1] = 0.0
    got = _run(inputs[:4] + (off,), L, grad)
    ref = spc.shade_pbr(*inputs[:4], off, L, grad)
    _check(got, ref, L.n, "light 1 switched off")
    two = spc.LightSet(L.vectors[[0, 2]], L.colors[[0, 2]], L.camera, L.ambient, (L.point[0], L.point[2]))
    without = _run(inputs[:4] + (np.ascontiguousarray(off[..., [0, 2]]),), two, grad)
    assert torch.equal(got["pixels"], without["pixels"])
    for name in ("positions", "colors", "normals", "material", "param_camera", "param_ambient"):
        assert np.array_equal(_bits(got["grads"][name]), _bits(without["grads"][name])), name
    assert not np.any(got["grads"]["param_vectors"][1]) and not np.any(got["grads"]["param_colors"][1])
    assert np.abs(ref["visibility"][..., 1]).max() > 0 and np.abs(got["grads"]["visibility"][..., 1]).max() > 0


def test_gradient_subsets():
    """Every subset of the per-pixel inputs with all and with no parameter, every subset of the parameters with all
    the per-pixel inputs: the requested gradients are bit-identical to the all-requested run's, the others None; the
    per-pixel gradients do not depend on whether a parameter is requested (one kernel with the sums, one without)."""
    inputs, L, grad, ref = spc.case("15x17-block_br")
    full = _run(inputs, L, grad)
    _check(full, ref, L.n, "all gradients")
    subsets = [(g, p) for g in itertools.product((False, True), repeat=5) for p in ((), PARAMS)]
    subsets += [((True,) * 5, tuple(n for n, on in zip(PARAMS, pick) if on))
                for pick in itertools.product((False, True), repeat=len(PARAMS))]
    for pix, params in subsets:
        got = _run(inputs, L, grad, pix, params)
        assert torch.equal(got["pixels"], full["pixels"])
        for name, need in list(zip(NAMES, pix)) + [("param_" + n, n in params) for n in PARAMS]:
            assert (got["grads"][name] is not None) == need, (pix, params, name)
        _same_grads(got, full, (pix, params))
        if any(pix) or params:
            assert _fused(got)


def test_nan_normal_invalidates_only_its_reach():
    """A NaN normal at a covered pixel on the silhouette: that pixel and the background neighbours whose window holds
    it are invalid; every output and gradient, the parameters' included, stays finite and as the statement's."""
    ident = "15x17-block_tl"  # covered rows 0..7, columns 0..8
    clean, L, grad, _ = spc.case(ident)
    pos, col, nrm, mat, vis = (a.copy() for a in clean)
    nrm[0, 7, 8, 1] = np.nan
    ref = spc.shade_pbr(pos, col, nrm, mat, vis, L, grad)
    for y, x0 in ((7, 8), (8, 7), (8, 8), (8, 9), (7, 9), (6, 9)):
        assert not ref["valid"][0, y, x0]
    assert ref["valid"][0, 6, 8] and ref["valid"][0, 5, 9]
    got = _run((pos, col, nrm, mat, vis), L, grad)
    _check(got, ref, L.n, "nan normal")
    assert all(np.all(np.isfinite(g)) for g in got["grads"].values()) and bool(torch.isfinite(got["pixels"]).all())


def test_nan_material_stays_at_its_pixel():
    """A NaN roughness at a lit interior pixel: NaN at that pixel and nowhere else (the material is read undilated,
    like the colour); a NaN material on the background, beside the silhouette, reaches no covered pixel."""
    ident = "15x17-block_tl"
    clean, L, grad, ref = spc.case(ident)
    lit = np.abs(ref["pixels"][0, :7, :8] - clean[1][0, :7, :8] * L.ambient).sum(-1) > 1e-3
    y, x0 = map(int, np.argwhere(lit)[0])
    mat = clean[3].copy()
    mat[0, y, x0, 0] = np.nan
    mat[0, 12, 12, 1] = np.nan  # background, out of every window's reach: invalid, never read
    got = _run(clean[:3] + (mat, clean[4]), L, grad, params=())
    pixels = got["pixels"].cpu().numpy()
    nan = np.isnan(pixels).any(-1)
    assert nan[0, y, x0] and nan.sum() == 1
    keep = ~nan
    assert np.array_equal(_bits(pixels[keep]), _bits(_run(clean, L, grad, params=())["pixels"].cpu().numpy()[keep]))
    for name in ("colors", "material", "visibility"):
        g = got["grads"][name]
        assert np.all(np.isfinite(g[keep])), name


def test_forms(monkeypatch):
    """[H,W,.] and non-contiguous inputs run the fused kernels and give the batched, contiguous result; float64,
    DIRT_FUSED_DEFERRED=0 and CPU tensors take the statement."""
    inputs, L, grad, ref = spc.case("15x17-island")
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
    wide_lights = torch.zeros((2, 6), device=DEV)
    wide_lights[:, ::2] = ps["vectors"].detach()
    wl = wide_lights.requires_grad_(True)
    ws = [w.requires_grad_(True) for w in wide]
    pixels, valid = _call([w[..., ::2] for w in ws], dict(ps, vectors=wl[:, ::2]), L)
    assert any("_ShadePbrFn" in x for x in _node_names(pixels))
    pixels.backward(_gpu(grad))
    assert torch.equal(pixels.detach(), base["pixels"]) and torch.equal(valid, base["valid"])
    for w, name in zip(ws, NAMES):
        assert np.array_equal(_bits(w.grad.cpu().numpy()[..., ::2]), _bits(base["grads"][name])), name
    assert np.array_equal(_bits(wl.grad.cpu().numpy()[:, ::2]), _bits(base["grads"]["param_vectors"]))

    def statement(got, tol_fwd):
        assert not _fused(got), got["nodes"]
        assert np.array_equal(got["valid"].cpu().numpy()[..., 0], ref["valid"])
        assert np.all(np.abs(got["pixels"].cpu().numpy() - ref["pixels"]) <= tol_fwd)

    f64 = _run(inputs, L, grad, dtype=torch.float64)
    statement(f64, 1e-12)
    for name, want in ref["params"].items():
        got = f64["grads"]["param_" + name].reshape(np.shape(want))
        assert np.abs(got - want).max() <= 1e-12 * max(1, np.abs(want).max())
    cpu = deferred.shade_pbr(*[torch.from_numpy(a) for a in inputs[:4]],
                             *[torch.from_numpy(x).requires_grad_(True) for x in (L.vectors, L.colors, L.camera)],
                             torch.from_numpy(L.ambient), L.point, torch.from_numpy(inputs[4]))
    assert "_ShadePbrFn" not in cpu[0].grad_fn.name() and cpu[0].device.type == "cpu"
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    statement(_run(inputs, L, grad), spc.fwd_bound(ref, L.n))


def test_double_backward_raises_on_the_fused_path():
    inputs, L, grad, ref = spc.case("15x17-hole")
    ts, ps = _tensors(inputs, L)
    pixels, _ = _call(ts, ps, L)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(pixels.square().sum(), [ps["vectors"]], create_graph=True)


def test_captures_into_a_graph():
    """One forward and backward with every gradient captured with torch.cuda.graph, replayed after every input changed
    in place: equal to the eager result bit for bit."""
    first, L1, grad, _ = spc.case("63x65-block_tl")
    second, L2 = spc.case("63x65-checkerboard")[0], spc.light_set("63x65-checkerboard")
    ts, ps = _tensors(first, L1)
    g = _gpu(grad)
    named = list(zip(NAMES, ts)) + [("param_" + n, p) for n, p in ps.items()]
    out = {}

    def step():
        pixels, valid = _call(ts, ps, L1)
        out["pixels"], out["valid"] = pixels, valid
        out["grads"] = torch.autograd.grad(pixels, [t for _, t in named], g)

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
    got = (out["pixels"].detach().clone(), out["valid"].clone(), [x.clone() for x in out["grads"]])
    del graph
    out.clear()
    eager = _run(second, L2, grad)
    assert L1.point == L2.point
    assert torch.equal(got[0], eager["pixels"]) and torch.equal(got[1], eager["valid"])
    for (name, _), a in zip(named, got[2]):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(eager["grads"][name])), name


def test_low_roughness():
    """tests/test_shade_pbr_cpu.py's low-roughness case (roughness in [0, 0.2), the clamp at R_MIN active): every
    output finite, the gradient to a roughness below R_MIN exactly 0, the forward within max(1, 2 W) of its bound, W
    the float32 framework ops' measured ratio there (the factor 2 covers the kernel's own operation order).  Measured
    on an MI355X: 3.517 of the bound against W = 2.32 and the limit 4.66."""
    inputs, L, grad, ref = low_roughness_case()
    got = _run(inputs, L, grad)
    assert _fused(got) and bool(torch.isfinite(got["pixels"]).all())
    assert all(np.all(np.isfinite(g)) for g in got["grads"].values())
    below = inputs[3][..., 0] < spc.R_MIN
    assert np.all(got["grads"]["material"][..., 0][below] == 0)
    v = ref["valid"]
    ratio = float((np.abs(got["pixels"].cpu().numpy() - ref["pixels"])[v] / spc.fwd_bound(ref, L.n)[v]).max())
    print("shade_pbr low roughness: forward %.3f of its bound (W = %.2f, limit %.2f)"
          % (ratio, LOW_ROUGHNESS_W, max(1.0, 2 * LOW_ROUGHNESS_W)))
    assert ratio <= max(1.0, 2 * LOW_ROUGHNESS_W)


# ---- the chain

def _chain(H=64, W=64):
    """camera G-buffers (positions, albedo, normals, uv) -> a 2-channel material texture fetched at the uv G-buffer ->
    one shadowed light's visibility at the dilated positions -> shade_pbr -> dp.loss_fn"""
    from test_gpu_shadow import CHAIN_BIAS, CHAIN_MAP, CHAIN_SOFTNESS, chain_scene
    world, faces, albedo, ML = chain_scene()
    f, al = _gpu(faces), _gpu(albedo)
    wts = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    tex0 = torch.rand((16, 16, 2), generator=torch.Generator().manual_seed(4)).to(DEV) * 0.6 + 0.3
    Vw, tex, M = _gpu(world).requires_grad_(True), tex0.requires_grad_(True), _gpu(ML)
    pos, col, nrm, clip = dp.gbuffers(dp.hip_render, Vw, f, al, H, W)
    vertex_uv = torch.stack([Vw[:, 0] / 2.8 + 0.5, Vw[:, 2] / 2.8 + 0.5], -1)
    uvbuf = dp.hip_render(torch.full((H, W, 2), float("-inf"), device=DEV), clip, vertex_uv, f, H, W, 2)
    material, sampled = deferred.sample_texture(tex, uvbuf)
    clip_l = torch.cat([Vw, torch.ones_like(Vw[:, :1])], -1) @ M
    S = CHAIN_MAP
    depth = dp.hip_render(torch.full((S, S, 1), float("inf"), device=DEV), clip_l, clip_l[:, 2:3], f, S, S, 1)
    vis, _ = deferred.sample_shadow(depth, deferred.dilate(pos), M, CHAIN_BIAS, CHAIN_SOFTNESS)
    lv = torch.tensor([[0., -1., 0.]], device=DEV)
    lc = torch.full((1, 3), 2.0, device=DEV)
    pixels, valid = deferred.shade_pbr(pos, col, nrm, material, lv, lc, dp.camera_position(H, W, DEV),
                                       torch.full((3,), 0.1, device=DEV), None, vis)
    loss = dp.loss_fn(pixels, valid, wts)
    g_v, g_tex, g_vis, g_mat = torch.autograd.grad(loss, [Vw, tex, vis, material])
    return dict(pixels=pixels.detach(), valid=valid, vis=vis.detach(), material=material, pixel_node=pixels,
                g_v=g_v, g_tex=g_tex, g_vis=g_vis, g_mat=g_mat)


def test_chain_material_texture_and_shadowed_light(monkeypatch):
    """The deferred chain at 64 x 64 (`_chain`): the fused ops against the statement path (DIRT_FUSED_DEFERRED=0:
    dilate, sample_texture, sample_shadow and shade_pbr all as framework ops) on the GPU.  valid equal; the gradients
    that reach the world vertices (the occluder's among them, through the shadow map), the material texture and the
    visibility within GRAD_FRAC of their scale (lighting_cases.grad_ratio).  Measured on an MI355X: pixels differ by at
    most 3.9e-7; d loss / d vertices 0.0016 of its bound (the occluder's 0.0011), d loss / d material texture 0.0066,
    d loss / d visibility 0.0087, d loss / d material 0.0252."""
    fused = _chain()
    assert any("_ShadePbrFn" in x for x in _node_names(fused["pixel_node"]))
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    ops = _chain()
    assert not any("_ShadePbrFn" in x for x in _node_names(ops["pixel_node"]))
    assert torch.equal(fused["valid"], ops["valid"]) and bool(fused["valid"].any()) and not bool(fused["valid"].all())
    shadowed = float((fused["vis"] < 0.5).float().mean())
    assert shadowed > 0.01
    n_surface = len(dp.grid_surface(n=12)[0])
    assert float(fused["g_v"][n_surface:].abs().max()) > 0 and float(fused["g_tex"].abs().max()) > 0
    ratios = {}
    for key in ("g_v", "g_tex", "g_vis", "g_mat"):
        ratios[key] = lighting_cases.grad_ratio(fused[key].cpu().numpy(), ops[key].cpu().numpy(), key)
    ratios["occluder"] = lighting_cases.grad_ratio(fused["g_v"][n_surface:].cpu().numpy(),
                                                   ops["g_v"][n_surface:].cpu().numpy(), "occluder")
    px = float((fused["pixels"] - ops["pixels"]).abs().max())
    print("pbr chain 64x64: %.1f %% of the pixels shadowed; pixels differ by at most %.3g; gradient ratios %s"
          % (100 * shadowed, px, {k: round(v, 4) for k, v in ratios.items()}))
    assert all(r <= 1.0 for r in ratios.values()), ratios
