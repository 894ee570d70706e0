"""deferred.reflect_view and deferred.shade_env on a CPU: the statement's vector-Jacobian products
(tests/shade_env_cases.py) against central differences in float64; the framework-op statements `_reflect_view_ops` and
`_shade_env_ops` against it in float64 (1e-12) and, in float32, within half of every bound the kernels are held to;
the clamps' ends; the agreement with shade_sh; the chain through the cube-map lookup; the six C entry points' argument
checks (no GPU call is made) and the public functions' errors.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import deferred_cases as dc
import lighting_cases
import shade_env_cases as sec
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_deferred_reflect_view_workspace", "dirt_deferred_reflect_view_fwd",
               "dirt_deferred_reflect_view_bwd", "dirt_deferred_shade_env_workspace", "dirt_deferred_shade_env_fwd",
               "dirt_deferred_shade_env_bwd")
NAMES = sec.PIXEL_NAMES
FRAC = lighting_cases.GRAD_FRAC


# ---- the statement's own derivatives

def _rows_inputs(seed=0, rows=8):
    """rows kept 0.05 away from the n.v kink, the q = e kink and the clamps' ends, both sides of each select present"""
    rng = np.random.default_rng(seed)
    cam = np.array([0.25, 1.75, 2.25])
    while True:
        p = rng.uniform(-1, 1, (rows, 3))
        nd = rng.standard_normal((rows, 3)) * rng.uniform(0.5, 2.0, (rows, 1))  # (not unit: u's Jacobian is exercised)
        c = rng.uniform(0.2, 1, (rows, 3))
        mat = np.stack([rng.uniform(0.1, 0.95, rows), rng.uniform(0.05, 0.95, rows)], -1)
        rad, occ = rng.uniform(0.1, 2, (rows, 3)), rng.uniform(0.2, 1, (rows, 1))
        coef = rng.uniform(-1, 1, (9, 3))
        t = sec.env_rows(p, nd, c, mat, rad, occ, None, coef, cam)
        if np.abs(t["nvr"]).min() > 0.05 and np.abs(t["qe"]).min() > 0.05 and (t["qe"] < 0).sum() >= 2 and \
                ((t["qe"] > 0) & (t["nvr"] > 0)).sum() >= 2 and (t["nvr"] < 0).sum() >= 1:
            return dict(p=p, nd=nd, c=c, mat=mat, rad=rad, occ=occ, coef=coef, cam=cam), rng.standard_normal((rows, 3))


def _central(loss, x, step=1e-6):
    num = np.zeros(x.shape)
    for idx in np.ndindex(*x.shape):
        hi, lo = x.copy(), x.copy()
        hi[idx] += step
        lo[idx] -= step
        num[idx] = (loss(hi) - loss(lo)) / (2 * step)
    return num


@pytest.mark.parametrize("K", sec.COUNTS)
def test_env_rows_vjp_against_central_differences(K):
    base, g = _rows_inputs()
    base["coef"] = base["coef"][:K]
    order = ("p", "nd", "c", "mat", "rad", "occ")
    ref = sec.env_rows(*[base[k] for k in order], g, base["coef"], base["cam"])

    def loss(**kw):
        a = dict(base, **kw)
        return (sec.env_rows(*[a[k] for k in order], None, a["coef"], a["cam"])["pixels"] * g).sum()
    for key, name, summed in (("p", "positions", False), ("nd", "normals", False), ("c", "colors", False),
                              ("mat", "material", False), ("rad", "radiance", False), ("occ", "occlusion", False),
                              ("coef", "coefficients", True), ("cam", "camera", True)):
        num = _central(lambda x: loss(**{key: x}), base[key])
        want = ref[name].sum(0) if summed else ref[name]
        assert np.abs(num - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), name


def test_reflect_rows_vjp_against_central_differences():
    base, g = _rows_inputs(1)
    ref = sec.reflect_rows(base["p"], base["nd"], g, base["cam"])
    assert np.abs(np.linalg.norm(ref["directions"], axis=-1) - 1).max() <= 1e-11

    def loss(**kw):
        a = dict(base, **kw)
        return (sec.reflect_rows(a["p"], a["nd"], None, a["cam"])["directions"] * g).sum()
    for key, name, summed in (("p", "positions", False), ("nd", "normals", False), ("cam", "camera", True)):
        num = _central(lambda x: loss(**{key: x}), base[key])
        want = ref[name].sum(0) if summed else ref[name]
        assert np.abs(num - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("ident,per_frame", [("2x2-hole", False), ("1x7-block_tl", False), ("3x5x6-leak", True)])
def test_whole_statements_against_central_differences(ident, per_frame):
    """Every gradient the two statements return -- the per-pixel inputs, positions and normals through the dilation,
    and each parameter -- against central differences of sum(output * grad).  The cases keep every pixel 1e-3 from the
    kinks, a thousand steps."""
    inputs, L, grad, ref = sec.case(ident, 9, per_frame)
    assert ref["valid"].any()
    f64 = [a.astype(np.float64) for a in inputs]

    class Wide(sec.Env):  # (float64: Env's float32 cast bypassed)
        def __init__(self, coefficients, camera):
            self.coefficients, self.camera, self.K = coefficients, camera, coefficients.shape[-2]

    def env_loss(i, x):
        args = list(f64)
        args[i] = x
        return (sec.shade_env(*args, L)["pixels"] * grad).sum()

    def central_where_finite(loss, x):
        num = np.zeros(x.shape)
        for idx in zip(*np.nonzero(np.isfinite(x))):
            vals = []
            for step in (1e-6, -1e-6):
                y = x.copy()
                y[idx] += step
                vals.append(loss(y))
            num[idx] = (vals[0] - vals[1]) / 2e-6
        return num
    for i, name in enumerate(NAMES):
        finite = np.isfinite(f64[i])
        num = central_where_finite(lambda x: env_loss(i, x), f64[i])
        want = np.where(finite, ref[name], 0.0)
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name
        assert not np.any(ref[name][~finite])
    wide = {"coefficients": L.coefficients.astype(np.float64), "camera": L.camera.astype(np.float64)}
    for name, want in ref["params"].items():
        num = _central(lambda x: (sec.shade_env(*inputs, Wide(**dict(wide, **{name: x})))["pixels"] * grad).sum(),
                       wide[name])
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name
    # reflect_view on the same frame
    p, n, camera, g, rref = sec.reflect_case(ident, per_frame)
    base = [p.astype(np.float64), n.astype(np.float64), camera.astype(np.float64)]
    for i, name in enumerate(("positions", "normals", "camera")):
        def loss(x):
            args = list(base)
            args[i] = x
            return (sec.reflect_view(*args)["directions"] * g).sum()
        want = rref["params"]["camera"] if name == "camera" else np.where(np.isfinite(base[i]), rref[name], 0.0)
        num = central_where_finite(loss, base[i])
        assert np.abs(num - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), name


# ---- the framework-op statements against the statement of record

def _t(a, dtype, dev="cpu", grad=True):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype).requires_grad_(grad)


def env_ops_run(inputs, L, grad, dtype, dev="cpu", fn=None):
    """-> (pixels, valid, {name: gradient as numpy}) of `_shade_env_ops` (or fn) with every gradient requested;
    inputs[5] None: no occlusion"""
    ts = [None if a is None else _t(a, dtype, dev) for a in inputs]
    ps = {"coefficients": _t(L.coefficients, dtype, dev), "camera": _t(L.camera, dtype, dev)}
    pixels, valid = (fn or deferred._shade_env_ops)(ts[0], ts[1], ts[2], ts[3], ps["coefficients"], ts[4],
                                                    ps["camera"], ts[5])
    named = [(n, t) for n, t in zip(NAMES, ts) if t is not None] + [("param_" + n, p) for n, p in ps.items()]
    grads = torch.autograd.grad(pixels, [t for _, t in named], _t(grad, dtype, dev, False), allow_unused=True)
    out = {n: (torch.zeros_like(t) if g is None else g).detach().cpu().numpy() for (n, t), g in zip(named, grads)}
    return pixels.detach().cpu().numpy(), valid.cpu().numpy(), out


def reflect_ops_run(p, n, camera, grad, dtype, dev="cpu", fn=None):
    ts = {"positions": _t(p, dtype, dev), "normals": _t(n, dtype, dev), "param_camera": _t(camera, dtype, dev)}
    directions, valid = (fn or deferred._reflect_view_ops)(*ts.values())
    grads = torch.autograd.grad(directions, list(ts.values()), _t(grad, dtype, dev, False), allow_unused=True)
    out = {k: (torch.zeros_like(t) if g is None else g).detach().cpu().numpy() for (k, t), g in zip(ts.items(), grads)}
    return directions.detach().cpu().numpy(), valid.cpu().numpy(), out


def _check_f64(run, ref, key, names, tag):
    out, valid, grads = run
    assert valid.shape == ref["valid"].shape + (1,) and np.array_equal(valid[..., 0], ref["valid"]), tag
    assert np.array_equal(out[~ref["valid"]], np.zeros_like(out[~ref["valid"]])), tag
    assert np.all(np.abs(out - ref[key]) <= 1e-12 * np.maximum(1.0, np.abs(ref[key]))), tag
    for name in names:
        if name in grads:
            assert np.all(np.isfinite(grads[name])), (tag, name)
            assert np.abs(grads[name] - ref[name]).max() <= 1e-12 * max(1.0, np.abs(ref[name]).max()), (tag, name)
    for name, want in ref["params"].items():
        got = grads["param_" + name].reshape(np.shape(want))
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (tag, name)


@pytest.mark.parametrize("ident", dc.FRAME_IDS)
def test_ops_match_the_statements_in_float64(ident):
    inputs, L, grad, ref = sec.case(ident)
    _check_f64(env_ops_run(inputs, L, grad, torch.float64), ref, "pixels", NAMES, ident)
    p, n, camera, g, rref = sec.reflect_case(ident)
    _check_f64(reflect_ops_run(p, n, camera, g, torch.float64), rref, "directions", ("positions", "normals"), ident)


@pytest.mark.parametrize("K", sec.COUNTS)
@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
def test_ops_coefficient_counts_and_per_frame_parameters_in_float64(K, per_frame):
    inputs, L, grad, ref = sec.case("3x5x6-leak", K, per_frame)
    assert L.coefficients.shape == ((3,) if per_frame else ()) + (K, 3)
    _check_f64(env_ops_run(inputs, L, grad, torch.float64), ref, "pixels", NAMES, (K, per_frame))
    if per_frame:  # the outer frames are all background
        for name in sec.PARAMS:
            assert np.all(ref["params"][name][[0, 2]] == 0) and np.abs(ref["params"][name][1]).max() > 0, name
        p, n, camera, g, rref = sec.reflect_case("3x5x6-leak", True)
        assert camera.shape == (3, 3)
        _check_f64(reflect_ops_run(p, n, camera, g, torch.float64), rref, "directions", ("positions", "normals"), K)


def test_no_occlusion_is_an_occlusion_of_ones_bit_for_bit():
    inputs, L, grad, _ = sec.case("15x17-island")
    ones = inputs[:5] + (np.ones_like(inputs[5]),)
    for dtype in (torch.float64, torch.float32):
        a = env_ops_run(ones, L, grad, dtype)
        b = env_ops_run(inputs[:5] + (None,), L, grad, dtype)
        assert np.array_equal(a[0], b[0])
        assert all(np.array_equal(a[2][k], b[2][k]) for k in b[2])
    ref1, ref0 = sec.shade_env(*ones, L, grad), sec.shade_env(*inputs[:5], None, L, grad)
    assert np.array_equal(ref1["pixels"], ref0["pixels"]) and np.array_equal(ref1["normals"], ref0["normals"])


def test_unbatched_statements_and_ops():
    inputs, L, grad, ref = sec.case("15x17-island")
    one = sec.shade_env(*(a[0] for a in inputs), L, grad[0])
    assert one["pixels"].shape == (15, 17, 3) and np.array_equal(one["pixels"], ref["pixels"][0])
    assert one["material"].shape == (15, 17, 2) and one["occlusion"].shape == (15, 17, 1)
    pixels, valid, grads = env_ops_run([a[0] for a in inputs], L, grad[0], torch.float64)
    assert pixels.shape == (15, 17, 3) and valid.shape == (15, 17, 1)
    assert np.abs(pixels - one["pixels"]).max() <= 1e-12
    assert np.abs(grads["material"] - one["material"]).max() <= 1e-12 * max(1.0, np.abs(one["material"]).max())
    p, n, camera, g, rref = sec.reflect_case("15x17-island")
    d, valid, grads = reflect_ops_run(p[0], n[0], camera, g[0], torch.float64)
    assert d.shape == (15, 17, 3) and valid.shape == (15, 17, 1) and np.abs(d - rref["directions"][0]).max() <= 1e-12


# ---- the bounds, on a CPU before any kernel is held to them

def env_bound_cases():
    """every case tests/test_gpu_shade_env.py holds to the statement's bounds -> [(tag, (inputs, Env, grad, ref))]"""
    out = [(i, sec.case(i)) for i in dc.FRAME_IDS]
    out += [("15x17-checkerboard K=%d" % K, sec.case("15x17-checkerboard", K)) for K in (1, 4)]
    out += [("leak per frame K=%d" % K, sec.case("3x5x6-leak", K, True)) for K in sec.COUNTS]
    out += [("no occlusion", sec.case("15x17-island", 9, False, False)), ("clamp ends", sec.clamp_ends_case())]
    for count in REDUCTION_COUNTS:
        out += [("1x%d" % count, sec.edge_case(1, count)),
                ("3x700 with %d valid" % count, sec.edge_case(3, 700, valid_count=count))]
    out += [("2x33x65 per_frame=%d" % pf, sec.edge_case(33, 65, B=2, seed=33, per_frame=pf, cover=0.7))
            for pf in (False, True)]
    return out


REDUCTION_COUNTS = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def env_measure(run, L, ref, tag, limit):
    """The worst ratios of one shade_env run against the three bounds -> (forward, per-pixel gradients, parameter
    gradients); each is asserted against `limit`"""
    pixels, valid, grads = run
    v = ref["valid"]
    assert np.array_equal(valid[..., 0], v), tag
    fwd = float((np.abs(pixels - ref["pixels"]) / sec.fwd_bound(ref, L.K)).max())
    assert fwd <= limit, (tag, "forward", fwd)
    worst_g = 0.0
    for name in NAMES:
        if grads.get(name) is not None:
            r = lighting_cases.grad_ratio(grads[name], ref[name], name)
            assert r <= limit, (tag, name, r)
            worst_g = max(worst_g, r)
    worst_p = 0.0
    for name, want in ref["params"].items():
        if grads.get("param_" + name) is not None:
            r = sec.param_ratio(grads["param_" + name], want, ref["absum"][name], FRAC)
            assert r <= limit, (tag, "param", name, r)
            worst_p = max(worst_p, r)
    return fwd, worst_g, worst_p


def reflect_measure(run, ref, tag, limit):
    directions, valid, grads = run
    assert np.array_equal(valid[..., 0], ref["valid"]), tag
    fwd = float((np.abs(directions - ref["directions"]) / sec.reflect_fwd_bound(ref)).max())
    assert fwd <= limit, (tag, "forward", fwd)
    worst_g = 0.0
    for name in ("positions", "normals"):
        if grads.get(name) is not None:
            r = lighting_cases.grad_ratio(grads[name], ref[name], name)
            assert r <= limit, (tag, name, r)
            worst_g = max(worst_g, r)
    worst_p = 0.0
    if grads.get("param_camera") is not None:
        worst_p = sec.param_ratio(grads["param_camera"], ref["params"]["camera"], ref["absum"]["camera"], FRAC)
        assert worst_p <= limit, (tag, "camera", worst_p)
    return fwd, worst_g, worst_p


def _report(what, worst):
    print("float32 framework ops, %s: forward %.3f at %s; per-pixel gradients %.3f at %s; parameter gradients %.3f "
          "at %s" % ((what,) + sum(worst, ())))


def test_float32_env_ops_stay_within_half_of_every_bound():
    """`_shade_env_ops` in float32 on the CPU against the forward bound (K + 2) FWD_ATOL + FWD_RTOL scale, the
    per-pixel gradient bound GRAD_FRAC of the tensor's scale and the parameter bound GRAD_FRAC * absum: at most 0.5
    on every case the GPU tests hold to the statement.  Measured: forward 0.016, per-pixel gradients 0.011, parameter
    gradients 0.019."""
    worst = [(0.0, None)] * 3
    for tag, (inputs, L, grad, ref) in env_bound_cases():
        got = env_measure(env_ops_run(inputs, L, grad, torch.float32), L, ref, tag, 0.5)
        worst = [max(w, (g, tag), key=lambda t: t[0]) for w, g in zip(worst, got)]
    _report("shade_env", worst)


def test_float32_reflect_ops_stay_within_half_of_every_bound():
    """`_reflect_view_ops` in float32 against 2 FWD_ATOL + FWD_RTOL, GRAD_FRAC of the gradients' scale and GRAD_FRAC *
    absum for the camera, over shade_env's cases' positions, normals and cameras.  Measured: forward 0.030, per-pixel
    gradients 0.005, the camera's 0.015."""
    worst = [(0.0, None)] * 3
    for tag, (inputs, L, _grad, _ref) in env_bound_cases():
        p, n, camera, g, ref = sec.reflect_case(tag) if tag in dc.FRAME_IDS else sec.reflect_of(inputs, L)
        got = reflect_measure(reflect_ops_run(p, n, camera, g, torch.float32), ref, tag, 0.5)
        worst = [max(w, (x, tag), key=lambda t: t[0]) for w, x in zip(worst, got)]
    _report("reflect_view", worst)


def test_cases_keep_their_distance_from_the_kinks():
    for tag, (inputs, L, _grad, ref) in env_bound_cases():
        if tag != "clamp ends" and inputs[5] is not None:
            assert sec.kink_distance(inputs, L) >= sec.MARGIN, tag
    covered = sum(int(ref["valid"].sum()) for _, (_, _, _, ref) in env_bound_cases())
    assert covered > 20000  # (no pixel is left out of a comparison: there is no mask in env_measure)


def test_reflection_has_unit_length_on_valid_pixels_and_is_zero_elsewhere():
    for ident in ("15x17-block_tl", "63x65-checkerboard", "3x5x6-leak", "7x1-all_background"):
        p, n, camera, g, ref = sec.reflect_case(ident)
        # (u(x) has the length |x| / (|x| + 1e-12), not 1: R is a few 1e-12 / |n_d| short of unit length in float64)
        for dtype, tol in ((torch.float64, 1e-10), (torch.float32, 1e-6)):
            d, valid, _ = reflect_ops_run(p, n, camera, g, dtype)
            length = np.linalg.norm(d.astype(np.float64), axis=-1)
            assert np.all(np.abs(length[valid[..., 0]] - 1.0) <= tol), ident
            assert np.array_equal(d[~valid[..., 0]], np.zeros_like(d[~valid[..., 0]])), ident
        assert np.all(np.abs(np.linalg.norm(ref["directions"], axis=-1)[ref["valid"]] - 1.0) <= 1e-10)
        assert not np.any(ref["directions"][~ref["valid"]])


def test_clamp_ends():
    """The material exactly on and past the clamps' ends (exactly representable values): the closed-interval
    derivative passes at roughness float32(0.045) and 1 and at metallic 0 and 1; a roughness of 0 (below R_MIN) and
    every value past an end get exactly 0, in the statement and in the ops in both dtypes."""
    inputs, L, grad, ref = sec.clamp_ends_case()
    v = ref["valid"]
    rough, metal = inputs[3][..., 0], inputs[3][..., 1]
    assert set(np.unique(rough)) == {0.0, float(np.float32(0.045)), 1.0, 1.5}
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, None)):
        run = env_ops_run(inputs, L, grad, dtype)
        if tol is None:
            env_measure(run, L, ref, "clamp ends", 0.5)
        g = run[2]["material"]
        for got in (g, ref["material"]):
            assert np.all(got[..., 0][(rough == 0.0) | (rough == 1.5)] == 0)
            assert np.all(got[..., 1][(metal == -0.5) | (metal == 1.5)] == 0)
            for on in (rough == np.float32(0.045), rough == 1.0):
                assert np.abs(got[..., 0][on & v]).min() > 0
            for on in (metal == 0.0, metal == 1.0):
                assert np.abs(got[..., 1][on & v]).min() > 0
        if tol is not None:
            assert np.abs(g - ref["material"]).max() <= tol * max(1.0, np.abs(ref["material"]).max())


def test_agrees_with_shade_sh_at_a_rough_dielectric():
    """metallic 0, roughness 1, radiance 0, occlusion 1: shade_env is shade_sh(colors, normals, coefficients,
    mask=the positions' background, normalize=True) on the pixels valid in both, to 1e-12 in float64."""
    for ident, K in (("15x17-block_br", 9), ("15x17-checkerboard", 4), ("7x1-island", 1), ("3x5x6-leak", 9)):
        inputs, L, _, ref = sec.case(ident, K)
        p, c, n = (torch.from_numpy(a).double() for a in inputs[:3])
        mat = torch.zeros(p.shape[:-1] + (2,), dtype=torch.float64)
        mat[..., 0] = 1.0
        coef, cam = torch.from_numpy(L.coefficients).double(), torch.from_numpy(L.camera).double()
        for occ in (None, torch.ones(p.shape[:-1] + (1,), dtype=torch.float64)):
            pixels, valid = deferred.shade_env(p, c, n, mat, coef, torch.zeros_like(p), cam, occ)
            want, valid_sh = deferred.shade_sh(c, n, coef, mask=torch.isinf(p).any(-1), normalize=True)
            both = (valid & valid_sh)[..., 0]
            assert np.array_equal(valid[..., 0].numpy(), ref["valid"]) and bool(both.any()) == bool(ref["valid"].any())
            assert np.abs((pixels - want)[both].numpy()).max(initial=0.0) <= 1e-12


def test_chain_leaves_unreached_background_out():
    """reflect_view -> _sample_cubemap_mip_ops -> shade_env on an 8 x 8 frame with a covered 3 x 3 block: the pixels
    the dilation does not reach get the direction (0, 0, 0), `valid` False and texel 0 from the lookup, and pixel 0
    with `valid` False from shade_env; no mask is passed anywhere."""
    rng = np.random.default_rng(8)
    covered = np.zeros((1, 8, 8), bool)
    covered[0, 1:4, 1:4] = True
    L = sec.draw_env(rng, 1)
    p, c, n, mat, rad, occ = (torch.from_numpy(a) for a in sec.settled_input(rng, covered, L))
    cam, coef = torch.from_numpy(L.camera), torch.from_numpy(L.coefficients)
    chain = deferred.build_cubemap_mipmaps(torch.rand((6, 8, 8, 3), generator=torch.Generator().manual_seed(1)) + 0.5)
    directions, valid = deferred.reflect_view(p, n, cam)
    radiance, sampled, _ = deferred._sample_cubemap_mip_ops(chain, directions, lod=mat[..., 0] * (len(chain) - 1))
    pixels, shaded = deferred.shade_env(p, c, n, mat, coef, radiance, cam, occlusion=occ)
    reached = np.zeros((8, 8), bool)
    reached[0:5, 0:5] = True
    assert np.array_equal(valid[0, ..., 0].numpy(), reached) and torch.equal(valid, shaded)
    assert torch.equal(sampled.reshape(valid.shape), valid)
    out = ~valid[..., 0]
    assert not bool(directions[out].any()) and not bool(radiance[out].any()) and not bool(pixels[out].any())
    assert bool((radiance[valid[..., 0]] > 0).all()) and bool(torch.isfinite(pixels).all())
    assert float(pixels[valid[..., 0]].abs().min()) > 0


# ---- the C entry points

def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "dirt_mi355x.h")).read()
    assert all(("int %s(" % n) in header for n in NEW_SYMBOLS)


def _workspace(op, B, H, W, K=None):
    size = ctypes.c_size_t(0)
    f = getattr(_lib.load(), "dirt_deferred_%s_workspace" % op)
    rc = f(B, H, W, ctypes.byref(size)) if K is None else f(B, H, W, K, ctypes.byref(size))
    assert rc == _lib.DIRT_OK
    return size.value


def _args(fn, B=1, H=4, W=4, K=9, null=(), workspace_short=0, want=("grad_positions", "grad_camera")):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    fits = 1 <= H <= _lib.MAX_DIM and 1 <= W <= _lib.MAX_DIM and K in (1, 4, 9)
    if "reflect_view" in fn:
        a = [p("positions"), p("normals"), B, H, W, 0, p("camera")]
        if fn.endswith("fwd"):
            return a + [p("directions"), p("valid"), p("route"), None], word
        size = _workspace("reflect_view", max(B, 0), H, W) if fits else 0
        outs = ("grad_positions", "grad_normals", "grad_camera")
    else:
        a = [p("positions"), p("colors"), p("normals"), p("material"), p("radiance"), p("occlusion"), B, H, W, K, 0,
             p("coefficients"), 0, p("camera")]
        if fn.endswith("fwd"):
            return a + [p("pixels"), p("valid"), p("route"), None], word
        size = _workspace("shade_env", max(B, 0), H, W, K) if fits else 0
        outs = ("grad_positions", "grad_colors", "grad_normals", "grad_material", "grad_radiance", "grad_occlusion",
                "grad_coefficients", "grad_camera")
    return a + [p("grad_pixels"), p("route")] + [p(o) if o in want else None for o in outs] + \
        [p("workspace"), size - workspace_short, None], word


def test_workspace_sizes():
    for B, H, W, K in ((1, 4, 4, 1), (1, 32, 32, 4), (2, 33, 65, 9), (0, 4, 4, 9), (3, 1, 257, 1)):
        assert _workspace("shade_env", B, H, W, K) == B * ((H * W + 255) // 256) * (3 + 3 * K) * 4
        assert _workspace("reflect_view", B, H, W) == B * ((H * W + 255) // 256) * 3 * 4
    lib, size = _lib.load(), ctypes.c_size_t(0)
    for K in (0, 2, 3, 5, 10):
        assert lib.dirt_deferred_shade_env_workspace(1, 4, 4, K, ctypes.byref(size)) == _lib.DIRT_EINVAL
        assert "coefficients" in lib.dirt_last_error().decode()
    assert lib.dirt_deferred_shade_env_workspace(1, 0, 4, 9, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_deferred_shade_env_workspace(1, 4, 4, 9, None) == _lib.DIRT_EINVAL
    assert lib.dirt_deferred_reflect_view_workspace(1, 4, _lib.MAX_DIM + 1, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_deferred_reflect_view_workspace(1, 4, 4, None) == _lib.DIRT_EINVAL


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    for fn in (s for s in NEW_SYMBOLS if not s.endswith("workspace")):
        f = getattr(lib, fn)
        op = "deferred_reflect_view" if "reflect_view" in fn else "deferred_shade_env"
        bads = [(dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=0), "height, width"),
                (dict(H=_lib.MAX_DIM + 1), "height, width"), (dict(W=_lib.MAX_DIM + 1), "height, width")]
        if op.endswith("env"):
            bads += [(dict(K=k), "coefficients") for k in (0, 2, 8, 10)]
        for bad, msg in bads:
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err() and op in err(), (fn, bad, err())
        # B == 0: nothing to do, whatever the pointers
        a, _keep = _args(fn, B=0, null=("positions", "pixels", "directions", "grad_pixels", "route", "camera",
                                        "workspace"))
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, H=0, null=("positions",))
        assert f(*a) == _lib.DIRT_EINVAL and "height, width" in err(), fn
    env = ("positions", "colors", "normals", "material", "radiance", "coefficients", "camera")
    required = {"dirt_deferred_reflect_view_fwd": ("positions", "normals", "camera", "directions", "valid", "route"),
                "dirt_deferred_reflect_view_bwd": ("positions", "normals", "camera", "grad_pixels", "route"),
                "dirt_deferred_shade_env_fwd": env + ("pixels", "valid", "route"),
                "dirt_deferred_shade_env_bwd": env + ("grad_pixels", "route")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    for fn in ("dirt_deferred_reflect_view_bwd", "dirt_deferred_shade_env_bwd"):
        f = getattr(lib, fn)
        # a workspace one byte short, or missing, with a parameter gradient requested
        for bad in (dict(workspace_short=1), dict(null=("workspace",))):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL and "workspace" in err(), (fn, bad)
        # ... nothing requested: no work and no error, whatever else is null
        a, _keep = _args(fn, want=(), null=("positions", "route", "workspace"))
        assert f(*a) == _lib.DIRT_OK, fn
    # the occlusion's gradient without an occlusion is nothing requested
    a, _keep = _args("dirt_deferred_shade_env_bwd", want=("grad_occlusion",), null=("occlusion", "positions"))
    assert lib.dirt_deferred_shade_env_bwd(*a) == _lib.DIRT_OK


# ---- the public functions

def test_public_surface_errors():
    assert set(deferred.__all__) == {"dilate", "shade"}
    assert callable(deferred.reflect_view) and callable(deferred.shade_env)
    g = [torch.zeros((4, 4, 3))] * 3
    mat, rad, coef, cam = torch.full((4, 4, 2), 0.5), torch.ones((4, 4, 3)), torch.ones((9, 3)), torch.ones(3)
    env = deferred.shade_env
    with pytest.raises(ValueError, match="shade_env: positions, colors, normals must share one shape"):
        env(g[0], g[1], torch.zeros((4, 3, 3)), mat, coef, rad, cam)
    with pytest.raises(ValueError, match="shade_env: material"):
        env(*g, torch.zeros((4, 4, 3)), coef, rad, cam)
    with pytest.raises(ValueError, match="shade_env: radiance"):
        env(*g, mat, coef, torch.ones((4, 4, 1)), cam)
    with pytest.raises(ValueError, match="shade_env: occlusion"):
        env(*g, mat, coef, rad, cam, occlusion=torch.ones((4, 4)))
    with pytest.raises(ValueError, match="shade_env: occlusion"):
        env(*g, mat, coef, rad, cam, occlusion=torch.ones((4, 4, 3)))
    with pytest.raises(ValueError, match=r"shade_env: coefficients must be \[K, 3\]"):
        env(*g, mat, torch.ones(9), rad, cam)
    with pytest.raises(ValueError, match="shade_env: 5 coefficients; K must be 1, 4 or 9"):
        env(*g, mat, torch.ones((5, 3)), rad, cam)
    with pytest.raises(ValueError, match="shade_env: per-frame coefficients"):
        env(*g, mat, torch.ones((1, 9, 3)), rad, cam)  # per-frame coefficients need a batch
    with pytest.raises(ValueError, match="shade_env: per-frame coefficients"):
        env(*[torch.zeros((2, 4, 4, 3))] * 3, torch.zeros((2, 4, 4, 2)), torch.ones((3, 9, 3)),
            torch.ones((2, 4, 4, 3)), cam)
    with pytest.raises(ValueError, match="shade_env: camera_position"):
        env(*g, mat, coef, rad, torch.ones((2, 3)))
    with pytest.raises(ValueError, match="reflect_view: camera_position"):
        deferred.reflect_view(g[0], g[2], torch.ones(4))
    with pytest.raises(ValueError, match="reflect_view: positions, normals must share one shape"):
        deferred.reflect_view(g[0], torch.zeros((4, 3, 3)), cam)
    with pytest.raises(ValueError, match="reflect_view: positions, normals must share one shape"):
        deferred.reflect_view(torch.zeros((4, 3)), torch.zeros((4, 3)), cam)
    pixels, valid = env(*g, mat, coef.tolist(), rad, [1.0, 1.0, 1.0])
    assert pixels.shape == (4, 4, 3) and valid.shape == (4, 4, 1) and bool(valid.all())
    directions, valid = deferred.reflect_view(g[0], torch.ones((4, 4, 3)), cam)
    assert directions.shape == (4, 4, 3) and valid.dtype == torch.bool and bool(valid.all())
    doc = " ".join(deferred.shade_env.__doc__.split())
    assert "read at the pixel itself" in doc and "`shade_sh`'s basis" in doc
    assert "reflect_view" in deferred.__doc__ and "shade_env" in deferred.__doc__


def test_statement_path_supports_double_backward():
    inputs, L, grad, ref = sec.case("15x17-hole")
    ts = [torch.from_numpy(a).double().requires_grad_(True) for a in inputs]
    coef = torch.from_numpy(L.coefficients).double().requires_grad_(True)
    cam = torch.from_numpy(L.camera).double().requires_grad_(True)
    pixels, _ = deferred.shade_env(ts[0], ts[1], ts[2], ts[3], coef, ts[4], cam, ts[5])
    gc, = torch.autograd.grad(pixels.square().sum(), [coef], create_graph=True)
    gg, gcam = torch.autograd.grad(gc.sum(), [ts[3], cam])
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0 and float(gcam.abs().max()) > 0
    directions, _ = deferred.reflect_view(ts[0], ts[2], cam)
    gn, = torch.autograd.grad((directions * torch.from_numpy(grad).double()).sum(), [ts[2]], create_graph=True)
    gg, = torch.autograd.grad(gn.square().sum(), [cam])
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0
