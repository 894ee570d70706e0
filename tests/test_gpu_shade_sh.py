"""The fused shade_sh kernels (dirt_amd/csrc/shade_sh_kernels.h through dirt_amd.deferred.shade_sh) against the float64
statement of record (tests/shade_sh_cases.py).

valid and the route word exact, invalid pixels exactly 0, valid pixels within K * FWD_ATOL + FWD_RTOL * scale (the
lighting contract per term, `scale` with the two cancelling basis terms taken uncancelled); the G-buffer gradients
within GRAD_FRAC of their reference's scale (tests/lighting_cases.py::grad_ratio); the coefficients' gradient within
GRAD_FRAC of the sum of its absolute per-pixel terms (`absum`; tests/test_shade_sh_cpu.py holds the framework ops in
float32 to half of each bound on the same cases); no frame left out of any check; every gradient bit-identical from
run to run.  Each test prints its worst measured ratios of error to bound.
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
import shade_sh_cases as shc
from dirt_amd import _lib, deferred

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAMES = ("colors", "normals", "coefficients")
FUSED = "_ShadeShFn"
CHUNK = 256  # kShThreads: the pixels one workgroup of the backward's first kernel owns


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _node_names(y):
    return [y.grad_fn.name()] + [fn.name() for fn, _ in y.grad_fn.next_functions if fn is not None]


def _run(colors, normals, coef, mask, normalize, grad, need=(True, True, True), dtype=torch.float32, fn=None):
    """-> dict: pixels, valid (tensors), nodes (names around pixels' grad_fn), grads {name: numpy, or None where no
    gradient was asked for}"""
    ts = [_gpu(a, dtype).requires_grad_(n) for a, n in zip((colors, normals, coef), need)]
    m = None if mask is None else _gpu(mask)
    pixels, valid = (fn or deferred.shade_sh)(*ts, m, normalize)
    wrt = [(n, t) for n, t in zip(NAMES, ts) if t.requires_grad]
    grads = dict.fromkeys(NAMES)
    if wrt:
        got = torch.autograd.grad(pixels, [t for _, t in wrt], _gpu(grad, dtype), allow_unused=True)
        for (n, t), g in zip(wrt, got):
            grads[n] = (torch.zeros_like(t) if g is None else g).cpu().numpy()
    torch.cuda.synchronize()
    return {"pixels": pixels.detach(), "valid": valid, "nodes": _node_names(pixels) if wrt else [], "grads": grads}


def _check(got, ref, K, tag):
    """-> worst ratios (forward, G-buffer gradients, coefficient gradient) of error to bound"""
    pixels, valid = got["pixels"].cpu().numpy(), got["valid"].cpu().numpy()
    assert valid.dtype == np.bool_ and valid.shape == ref["valid"].shape + (1,), tag
    assert np.array_equal(valid[..., 0], ref["valid"]), tag
    v = ref["valid"]
    assert np.array_equal(pixels[~v], np.zeros_like(pixels[~v])), tag
    err, bound = np.abs(pixels - ref["pixels"])[v], shc.fwd_bound(ref, K)[v]
    fwd = float((err / bound).max()) if err.size else 0.0
    assert fwd <= 1.0, (tag, fwd)
    worst_g = worst_c = 0.0
    for name in NAMES[:2]:
        if got["grads"][name] is not None:
            r = lighting_cases.grad_ratio(got["grads"][name], ref[name], "%s d %s" % (tag, name))
            assert r <= 1.0, (tag, name, r)
            worst_g = max(worst_g, r)
    g = got["grads"]["coefficients"]
    if g is not None:
        assert g.shape == ref["coefficients"].shape and np.all(np.isfinite(g)), tag
        worst_c = shc.param_ratio(g, ref["coefficients"], ref["absum"])
        assert worst_c <= 1.0, (tag, worst_c)
    print("shade_sh %s: forward %.4f of its bound, G-buffer gradients %.4f, coefficient gradient %.4f of theirs"
          % (tag, fwd, worst_g, worst_c))
    return fwd, worst_g, worst_c


def _same_grads(a, b, tag):
    for name in NAMES:
        if a["grads"][name] is None or b["grads"].get(name) is None:
            continue
        assert np.array_equal(_bits(a["grads"][name]), _bits(b["grads"][name])), (tag, name)


def _fused_twice(colors, normals, coef, mask, normalize, grad, ref, K, tag):
    """the usual: the fused node, all gradients, against the statement, a second run with the same bits"""
    got = _run(colors, normals, coef, mask, normalize, grad)
    assert any(FUSED in n for n in got["nodes"]), got["nodes"]
    assert not got["valid"].requires_grad
    _check(got, ref, K, tag)
    again = _run(colors, normals, coef, mask, normalize, grad)
    assert torch.equal(got["pixels"], again["pixels"])
    _same_grads(got, again, tag)
    return got


def _raw_fwd(colors, normals, coef, mask, normalize):
    """dirt_deferred_shade_sh_fwd itself -> (pixels, valid uint8 [B,H,W], route int32) tensors and the inputs"""
    ts = [_gpu(a) for a in (colors, normals, coef)]
    m = None if mask is None else _gpu(np.asarray(mask) != 0).view(torch.uint8)
    B, H, W, _ = ts[0].shape
    pixels = torch.empty_like(ts[0])
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    route = torch.empty((B, H, W), dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().dirt_deferred_shade_sh_fwd(
        ts[0].data_ptr(), ts[1].data_ptr(), None if m is None else m.data_ptr(), B, H, W, coef.shape[-2],
        int(coef.ndim == 3), ts[2].data_ptr(), int(normalize), pixels.data_ptr(), valid.data_ptr(), route.data_ptr(),
        torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return pixels, valid, route, ts


def _raw_route(colors, normals, coef, mask, normalize):
    return _raw_fwd(colors, normals, coef, mask, normalize)[2].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_matches_the_statement(ident):
    """K = 9, raw normals, over the table of edge frames, every gradient requested."""
    colors, normals, coef, mask, grad, ref = shc.case(ident)
    got = _fused_twice(colors, normals, coef, mask, False, grad, ref, 9, ident)
    assert np.array_equal(_raw_route(colors, normals, coef, mask, False), ref["route"]), ident
    if ident.endswith("all_background"):
        assert not got["pixels"].any() and not got["valid"].any()
        for name, g in got["grads"].items():
            assert not np.any(g), (ident, name)  # exactly 0


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("K", shc.COUNTS)
def test_coefficient_counts_forms_and_normalisation(K, normalize, per_frame):
    for ident in ("15x17-checkerboard", "3x5x6-leak"):
        colors, normals, coef, mask, grad, ref = shc.case(ident, K, per_frame, False, normalize)
        got = _fused_twice(colors, normals, coef, mask, normalize, grad, ref, K,
                           "%s K=%d normalize=%d per_frame=%d" % (ident, K, normalize, per_frame))
        assert np.array_equal(_raw_route(colors, normals, coef, mask, normalize), ref["route"])
        if per_frame and ident == "3x5x6-leak":  # the outer frames are all background
            g = got["grads"]["coefficients"]
            assert g.shape == (3, K, 3) and not np.any(g[[0, 2]]) and np.any(g[1])


def _edge_case(H, W, B=1, valid_count=None, K=9, per_frame=False, normalize=False, seed=0):
    """A fully covered frame (valid_count: only its first pixels have a usable normal) and its inputs"""
    rng = np.random.default_rng([seed, H, W, B, valid_count or 0])
    covered = np.ones((B, H, W), bool)
    invalid = None
    if valid_count is not None:
        invalid = (np.arange(H * W) >= valid_count).reshape(1, H, W).repeat(B, 0)
    colors, normals = shc.random_input(rng, covered, invalid, (0.3, 1.5) if normalize else None)
    coef = shc.draw_coefficients(rng, K, B if per_frame else None)
    grad = rng.standard_normal(colors.shape).astype(np.float32)
    return colors, normals, coef, grad


@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_reduction_edges(count):
    """Frames of `count` pixels, and `count` valid pixels in a larger frame: a wave, a workgroup (which is a chunk)
    and four chunks, each one pixel short, full, and one over."""
    for H, W, valid_count in ((1, count, None), (3, 700, count)):
        colors, normals, coef, grad = _edge_case(H, W, valid_count=valid_count)
        ref = shc.shade_sh(colors, normals, coef, None, False, grad)
        assert int(ref["valid"].sum()) == count
        _fused_twice(colors, normals, coef, None, False, grad, ref, 9, "%dx%d with %d valid" % (H, W, count))


def test_two_frames_of_several_ragged_chunks():
    """33 x 65 = 2145 pixels: nine chunks a frame, the last one ragged, in each of two frames"""
    rng = np.random.default_rng(33)
    covered = rng.random((2, 33, 65)) < 0.7
    colors, normals = shc.random_input(rng, covered, None, (0.3, 1.5))
    grad = rng.standard_normal(colors.shape).astype(np.float32)
    for per_frame in (False, True):
        coef = shc.draw_coefficients(rng, 9, 2 if per_frame else None)
        ref = shc.shade_sh(colors, normals, coef, None, True, grad)
        _fused_twice(colors, normals, coef, None, True, grad, ref, 9, "2x33x65 per_frame=%d" % per_frame)


def test_more_chunks_than_the_second_kernel_has_threads():
    """512 x 513: 1026 chunks, four times the reducing workgroup's 256 threads and two over.  Against `_shade_sh_ops`
    in float64 on the GPU; absum and scale (the bounds' scales) from the statement, which is plain numpy here: the
    frame has one background row only."""
    rng = np.random.default_rng(512)
    covered = np.ones((1, 512, 513), bool)
    covered[0, 300] = False
    colors, normals = shc.random_input(rng, covered)
    coef = shc.draw_coefficients(rng, 9)
    grad = rng.standard_normal(colors.shape).astype(np.float32)
    got = _run(colors, normals, coef, None, False, grad)
    assert any(FUSED in n for n in got["nodes"])
    want = _run(colors, normals, coef, None, False, grad, dtype=torch.float64, fn=deferred._shade_sh_ops)
    stmt = shc.shade_sh(colors, normals, coef, None, False, grad)
    assert np.array_equal(want["valid"].cpu().numpy()[..., 0], stmt["valid"])
    ref = dict(stmt, pixels=want["pixels"].cpu().numpy(), **want["grads"])
    _check(got, ref, 9, "512x513")
    _same_grads(got, _run(colors, normals, coef, None, False, grad), "512x513")


def _raw_bwd(colors, normals, coef, normalize, grad, with_coefficients):
    """dirt_deferred_shade_sh_fwd for the route, then dirt_deferred_shade_sh_bwd itself into buffers (the workspace
    included) pre-filled with NaN: whatever the launches leave unwritten stays NaN.  -> {name: numpy}"""
    _, _, route, ts = _raw_fwd(colors, normals, coef, None, normalize)
    B, H, W, _ = ts[0].shape
    K = coef.shape[-2]
    lib, stream = _lib.load(), torch.cuda.current_stream(DEV).cuda_stream
    out = {name: torch.full_like(t, float("nan")) for name, t in zip(NAMES[:2], ts)}
    workspace, size = None, _lib._SZ(0)
    if with_coefficients:
        out["coefficients"] = torch.full_like(ts[2], float("nan"))
        _lib.check(lib.dirt_deferred_shade_sh_workspace(B, H, W, K, ctypes.byref(size)))
        assert size.value == B * -(-H * W // CHUNK) * 3 * K * 4  # (7 MB at 65,537 frames and nine coefficients)
        workspace = torch.full((size.value // 4,), float("nan"), device=DEV)
    ptr = lambda name: out[name].data_ptr() if name in out else None  # noqa: E731
    g = _gpu(grad)
    _lib.check(lib.dirt_deferred_shade_sh_bwd(
        ts[0].data_ptr(), ts[1].data_ptr(), B, H, W, K, int(coef.ndim == 3), ts[2].data_ptr(), int(normalize),
        g.data_ptr(), route.data_ptr(), ptr("colors"), ptr("normals"), ptr("coefficients"),
        None if workspace is None else workspace.data_ptr(), size.value, stream))
    torch.cuda.synchronize()
    assert workspace is None or bool(torch.isfinite(workspace).all())  # every partial row was written
    res = dict.fromkeys(NAMES)
    res.update({name: t.cpu().numpy() for name, t in out.items()})
    return res


MANY_FRAMES = 65537  # two more than a grid's second dimension holds


@functools.lru_cache(maxsize=None)
def _many_frames_case(per_frame):
    """65,537 frames of 1 x 3 pixels, every seventh with one background pixel; the cotangent is nonzero in the frames
    of S alone (both ends, the two sides of the grid's 65,535, the middle, five drawn ones).  The statement's frames
    are independent: it is evaluated on the frames of S, with per-frame coefficients sliced to them.  A frame whose
    cotangent is zero adds exact zeros to a shared gradient, so the statement's sums over S are the batch's."""
    B = MANY_FRAMES
    rng = np.random.default_rng([65537, int(per_frame)])
    S = np.array(sorted({0, 1, 32767, 65534, 65535, 65536} | set(rng.choice(B, 5, replace=False).tolist())))
    covered = np.ones((B, 1, 3), bool)
    covered[::7, 0, 1] = False
    assert (~covered[S]).any() and covered[S].all(-1).any()
    colors, normals = shc.random_input(rng, covered, None, (0.3, 1.5))
    coef = shc.draw_coefficients(rng, 9, B if per_frame else None)
    grad = np.zeros(colors.shape, np.float32)
    grad[S] = rng.standard_normal(grad[S].shape).astype(np.float32)
    ref = shc.shade_sh(colors[S], normals[S], coef[S] if per_frame else coef, None, True, grad[S])
    assert (ref["valid"] & ~covered[S]).any()  # (background pixels that the dilation fills: routes other than own)
    return colors, normals, coef, grad, S, ref


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
def test_more_frames_than_a_grids_y_extent(per_frame):
    """The backward's first kernel walks `for (frame = blockIdx.y; frame < B; frame += gridDim.y)` under a grid of
    min(B, 65535) rows: at 65,537 frames the workgroups of rows 0 and 1 iterate twice, re-using their LDS sums.  With
    the coefficients' gradient (the summing kernel and the reduction) and without, through autograd and through the
    entry point itself into NaN-filled buffers: forward, route and every gradient on the frames of S against the
    statement, exact zeros in every other frame, bit-identical from run to run."""
    colors, normals, coef, grad, S, ref = _many_frames_case(per_frame)
    B = MANY_FRAMES
    others = np.ones(B, bool)
    others[S] = False
    framed = NAMES[:2] + (("coefficients",) if per_frame else ())
    assert np.array_equal(_raw_route(colors, normals, coef, None, True)[S], ref["route"])
    tag = "%d frames, %s coefficients" % (B, "per-frame" if per_frame else "shared")

    def on_S(grads, pixels, valid):
        for name in framed:
            if grads.get(name) is not None:
                assert grads[name].shape[0] == B and not np.any(grads[name][others]), (tag, name)  # exactly 0
        at = torch.from_numpy(S).to(DEV)
        return {"pixels": pixels[at], "valid": valid[at],
                "grads": {k: (g[S] if k in framed and g is not None else g) for k, g in grads.items()}}

    full = _run(colors, normals, coef, None, True, grad)
    assert any(FUSED in n for n in full["nodes"])
    _check(on_S(full["grads"], full["pixels"], full["valid"]), ref, 9, tag + ", all gradients")
    _same_grads(full, _run(colors, normals, coef, None, True, grad), tag)
    plain = _run(colors, normals, coef, None, True, grad, need=(True, True, False))
    _check(on_S(plain["grads"], plain["pixels"], plain["valid"]), ref, 9, tag + ", G-buffers alone")
    _same_grads(full, plain, tag)
    for with_coefficients in (True, False):
        raw = _raw_bwd(colors, normals, coef, True, grad, with_coefficients)
        assert all(np.all(np.isfinite(g)) for g in raw.values() if g is not None), tag  # nothing stays NaN
        _check(on_S(raw, full["pixels"], full["valid"]), ref, 9, tag + ", raw, coefficients=%d" % with_coefficients)
        _same_grads(full, {"grads": raw}, tag)


def test_gradient_subsets():
    """Every subset of {colors, normals, coefficients}: the requested gradients are bit-identical to the all-requested
    run's, the others None (the G-buffer gradients do not depend on whether the sums run)."""
    colors, normals, coef, mask, grad, ref = shc.case("15x17-block_br", 9, False, False, True)
    full = _run(colors, normals, coef, mask, True, grad)
    _check(full, ref, 9, "all gradients")
    for need in itertools.product((False, True), repeat=3):
        got = _run(colors, normals, coef, mask, True, grad, need)
        assert torch.equal(got["pixels"], full["pixels"]) and torch.equal(got["valid"], full["valid"])
        for name, n in zip(NAMES, need):
            assert (got["grads"][name] is not None) == n, (need, name)
        _same_grads(got, full, need)
        if any(need):
            assert any(FUSED in x for x in got["nodes"])


def test_explicit_mask_that_differs_from_the_default():
    for normalize in (False, True):
        colors, normals, coef, mask, grad, ref = shc.case("63x65-block_tl", 9, False, True, normalize)
        default = shc.case("63x65-block_tl", 9, False, False, normalize)[5]
        assert not np.array_equal(ref["route"], default["route"]) and not np.array_equal(ref["valid"], default["valid"])
        _fused_twice(colors, normals, coef, mask, normalize, grad, ref, 9, "explicit mask, normalize=%d" % normalize)
        assert np.array_equal(_raw_route(colors, normals, coef, mask, normalize), ref["route"])
        as_bool = _run(colors, normals, coef, mask.astype(bool), normalize, grad)
        as_float = _run(colors, normals, coef, mask.astype(np.float32) * 0.5, normalize, grad)
        for other in (as_bool, as_float):
            assert torch.equal(other["valid"], as_bool["valid"]) and any(FUSED in x for x in other["nodes"])
            _check(other, ref, 9, "explicit mask, another dtype")


def test_nan_normal_invalidates_only_its_reach():
    """A NaN normal at a covered pixel on the silhouette: that pixel and the background neighbours whose window holds
    it are invalid; every output and gradient, the coefficients' included, stays finite and as the statement's."""
    ident = "15x17-block_tl"  # covered rows 0..7, columns 0..8
    colors, clean, coef, _, grad, _ = shc.case(ident)
    normals = clean.copy()
    normals[0, 7, 8, 1] = np.nan
    ref = shc.shade_sh(colors, normals, coef, None, False, grad)
    for y, x0 in ((7, 8), (8, 7), (8, 8), (8, 9), (7, 9), (6, 9)):
        assert not ref["valid"][0, y, x0]
    assert ref["valid"][0, 6, 8] and ref["valid"][0, 5, 9]
    got = _fused_twice(colors, normals, coef, None, False, grad, ref, 9, "nan normal")
    assert all(np.all(np.isfinite(g)) for g in got["grads"].values()) and bool(torch.isfinite(got["pixels"]).all())


def test_normalised_normal_lengths():
    """normalize=True with lengths 0.3 .. 1.5 on the larger frames of the table"""
    for ident in ("63x65-checkerboard", "16x256-block_br", "63x65-island"):
        colors, normals, coef, mask, grad, ref = shc.case(ident, 9, False, False, True)
        lengths = np.linalg.norm(normals[np.isfinite(normals).all(-1)].astype(np.float64), axis=-1)
        assert lengths.min() >= 0.29 and lengths.max() <= 1.51 and (lengths.max() > 1.2 or lengths.size < 4)
        _fused_twice(colors, normals, coef, mask, True, grad, ref, 9, ident + " normalized")


def test_zero_normal_takes_the_subgradient():
    """A covered pixel whose normal is exactly 0 under normalize=True: u = 0.  With bands 0-1 its pixel is colors *
    coefficients[0] * c0 (with band 2, Y6 = -c3 at u = 0 adds its term: K = 9 is held to the statement instead); its
    grad_normals is g_u / (0 + 1e-12): finite, and within BIG_ROW_RTOL of its own scale."""
    for K in (4, 9):
        colors, clean, coef, _, grad, _ = shc.case("15x17-no_background", K, False, False, True)
        normals = clean.copy()
        normals[0, 7, 8] = 0.0
        ref = shc.shade_sh(colors, normals, coef, None, True, grad)
        assert ref["valid"][0, 7, 8]
        got = _run(colors, normals, coef, None, True, grad)
        assert any(FUSED in n for n in got["nodes"])
        pixels = got["pixels"].cpu().numpy()
        v = ref["valid"]
        assert np.array_equal(got["valid"].cpu().numpy()[..., 0], v)
        assert np.all(np.abs(pixels - ref["pixels"])[v] <= shc.fwd_bound(ref, K)[v])
        if K == 4:
            want = colors[0, 7, 8].astype(np.float64) * coef[0].astype(np.float64) * shc.C0
            assert np.all(np.abs(pixels[0, 7, 8] - want) <= shc.fwd_bound(ref, K)[0, 7, 8])
        gn = got["grads"]["normals"]
        assert np.all(np.isfinite(gn)) and np.abs(ref["normals"][0, 7, 8]).max() > 1e9
        row = 7 * 17 + 8
        r = lighting_cases.grad_ratio(gn, ref["normals"], "zero normal", big_rows=(row,))
        rc = lighting_cases.grad_ratio(got["grads"]["colors"], ref["colors"], "zero normal, colours")
        rk = shc.param_ratio(got["grads"]["coefficients"], ref["coefficients"], ref["absum"])
        print("shade_sh zero normal K=%d: normals %.4f of the bound (its row apart), colours %.4f, coefficients %.4f"
              % (K, r, rc, rk))
        assert r <= 1.0 and rc <= 1.0 and rk <= 1.0
        _same_grads(got, _run(colors, normals, coef, None, True, grad), "zero normal")


def test_forms(monkeypatch):
    """[H,W,3] and non-contiguous inputs run the fused kernels and give the batched, contiguous bits; float64,
    DIRT_FUSED_DEFERRED=0 and CPU tensors take the statement."""
    colors, normals, coef, mask, grad, ref = shc.case("15x17-island", 9, False, False, True)
    base = _run(colors, normals, coef, None, True, grad)
    one = _run(colors[0], normals[0], coef, None, True, grad[0])
    assert one["pixels"].shape == (15, 17, 3) and one["valid"].shape == (15, 17, 1)
    assert any(FUSED in x for x in one["nodes"])
    assert torch.equal(one["pixels"], base["pixels"][0]) and torch.equal(one["valid"], base["valid"][0])
    for name in NAMES:
        assert np.array_equal(_bits(one["grads"][name]).reshape(-1), _bits(base["grads"][name]).reshape(-1)), name
    wide = [torch.zeros((1, 15, 17, 6), device=DEV) for _ in range(2)]
    for w, a in zip(wide, (colors, normals)):
        w[..., ::2] = _gpu(a)
    wide_coef = torch.zeros((9, 6), device=DEV)
    wide_coef[:, ::2] = _gpu(coef)
    ws = [w.requires_grad_(True) for w in wide + [wide_coef]]
    pixels, valid = deferred.shade_sh(ws[0][..., ::2], ws[1][..., ::2], ws[2][:, ::2], None, True)
    assert any(FUSED in x for x in _node_names(pixels))
    pixels.backward(_gpu(grad))
    assert torch.equal(pixels.detach(), base["pixels"]) and torch.equal(valid, base["valid"])
    for w, name in zip(ws, NAMES):
        assert np.array_equal(_bits(w.grad.cpu().numpy()[..., ::2]), _bits(base["grads"][name])), name

    def statement(got, tol_fwd):
        assert not any(FUSED in x for x in got["nodes"]), got["nodes"]
        assert np.array_equal(got["valid"].cpu().numpy()[..., 0], ref["valid"])
        assert np.all(np.abs(got["pixels"].cpu().numpy() - ref["pixels"]) <= tol_fwd)

    f64 = _run(colors, normals, coef, None, True, grad, dtype=torch.float64)
    statement(f64, 1e-12)
    for name in NAMES:
        assert np.abs(f64["grads"][name] - ref[name]).max() <= 1e-12 * max(1, np.abs(ref[name]).max()), name
    cpu = deferred.shade_sh(torch.from_numpy(colors), torch.from_numpy(normals),
                            torch.from_numpy(coef).requires_grad_(True), None, True)
    assert FUSED not in cpu[0].grad_fn.name() and cpu[0].device.type == "cpu"
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    statement(_run(colors, normals, coef, None, True, grad), shc.fwd_bound(ref, 9))


def test_double_backward_raises_on_the_fused_path_and_works_on_the_statement(monkeypatch):
    colors, normals, coef, mask, grad, ref = shc.case("15x17-hole", 9, False, False, True)
    ts = [_gpu(a).requires_grad_(True) for a in (colors, normals, coef)]
    pixels, _ = deferred.shade_sh(*ts, None, True)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(pixels.square().sum(), [ts[2]], create_graph=True)
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    pixels, _ = deferred.shade_sh(*ts, None, True)
    gc_, = torch.autograd.grad(pixels.square().sum(), [ts[2]], create_graph=True)
    gg, = torch.autograd.grad(gc_.sum(), [ts[1]])
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0


def test_captures_into_a_graph():
    """One forward and backward with every gradient captured with torch.cuda.graph (one stream, no parallel branches),
    replayed after the G-buffers and the coefficients changed in place: equal to the eager result bit for bit."""
    c1, n1, k1, _, grad, _ = shc.case("63x65-block_tl", 9, False, False, True)
    c2, n2, k2 = shc.case("63x65-checkerboard", 9, False, False, True)[:3]
    ts = [_gpu(a).requires_grad_(True) for a in (c1, n1, k1)]
    g = _gpu(grad)
    out = {}

    def step():
        pixels, valid = deferred.shade_sh(*ts, None, True)
        out["pixels"], out["valid"] = pixels, valid
        out["grads"] = torch.autograd.grad(pixels, ts, g)

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
        for t, a in zip(ts, (c2, n2, k2)):
            t.copy_(_gpu(a))
    graph.replay()
    torch.cuda.synchronize()
    got = (out["pixels"].detach().clone(), out["valid"].clone(), [x.clone() for x in out["grads"]])
    del graph
    out.clear()
    eager = _run(c2, n2, k2, None, True, grad)
    assert torch.equal(got[0], eager["pixels"]) and torch.equal(got[1], eager["valid"])
    for name, a in zip(NAMES, got[2]):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(eager["grads"][name])), name


def test_end_to_end_from_a_rasterised_mesh():
    """rasterise a small surface's normals (over -inf) and albedo (over 0) at 32 x 32, shade_sh, a sum loss: the fused
    result and `_shade_sh_ops` in float64 on the same G-buffers agree within the bounds; the vertex gradient through
    the rasteriser is finite and nonzero."""
    import deferred_pipeline as dp
    world, faces, albedo = dp.grid_surface(8)
    vertices = _gpu(world).requires_grad_(True)
    _, colors, normals, _ = dp.gbuffers(dp.hip_render, vertices, _gpu(faces), _gpu(albedo), 32, 32)
    assert bool(torch.isinf(normals).any()) and bool(torch.isfinite(normals).all(-1).any())
    coef = _gpu(shc.draw_coefficients(np.random.default_rng(8), 9)).requires_grad_(True)
    pixels, valid = deferred.shade_sh(colors, normals, coef, None, True)
    assert any(FUSED in n for n in _node_names(pixels))
    g_vertices, g_coef = torch.autograd.grad(pixels.sum(), [vertices, coef])
    assert bool(torch.isfinite(g_vertices).all()) and float(g_vertices.abs().max()) > 0
    cn, nn, kn = (t.detach().cpu().numpy() for t in (colors, normals, coef))
    ones = np.ones(cn.shape, np.float32)
    stmt = shc.shade_sh(cn, nn, kn, None, True, ones)
    want = _run(cn, nn, kn, None, True, ones, dtype=torch.float64, fn=deferred._shade_sh_ops)
    assert np.array_equal(want["valid"].cpu().numpy()[..., 0], stmt["valid"])
    ref = dict(stmt, pixels=want["pixels"].cpu().numpy(), **want["grads"])
    got = {"pixels": pixels.detach(), "valid": valid,
           "grads": {"colors": None, "normals": None, "coefficients": g_coef.cpu().numpy()}}
    _check(got, ref, 9, "end to end 32x32")
    leaf = _run(cn, nn, kn, None, True, ones)
    _check(leaf, ref, 9, "end to end 32x32, G-buffer gradients")
