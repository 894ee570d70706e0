"""CPU pin of the lighting helpers: the float64 statement (tests/lighting_f64.py) against central differences, and
the framework-op statement (dirt_amd/lighting.py `_*_ops`) against it on every edge case of
tests/lighting_cases.py -- the same table tests/test_gpu_lighting_f64.py holds the fused HIP kernels to.

  * Self-check: every vector-Jacobian product of the statement (the light parameters' and the shininess's
    included) against central differences in float64 at smooth points (|cos| > 0.2, a non-degenerate grid mesh),
    step 1e-6 on operands of order 1.  Bound 1e-6 of the gradient's scale; measured 7.7e-11 (vertex_normals),
    1.3e-10 (diffuse_directional), 1.4e-8 (specular_directional, at k = 0.5), 4.2e-10 (diffuse_point).
  * `_*_ops` in float64 on a CPU match the statement within 1e-12 of scale, forward and every gradient (the light
    parameters' and a tensor shininess's included): this pins the formulas.  Measured at most 1.1e-14.
  * `_*_ops` in float32 on a CPU stay within A THIRD of the project's float32 contract (forward 2e-6 + 1e-5 |ref|,
    gradients 1e-4 of scale; tests/test_gpu_lighting.py), so that the contract can hold the GPU kernels on the same
    cases.  The cases were sized for that, never the tolerance: the fan stops at valence 512 (a float32 sum of
    thousands of unit normals does not keep 1e-5) and its apex height is a power of two (lighting_cases._fan); the
    shininess rows carry no cancellation in cos (lighting_cases.shininess_cases).

Measured float32 maxima of the framework ops on a CPU, as fractions of the contract (forward, gradients), per
group of cases; the fused kernels' on an MI355X in brackets:
    sizes, diffuse_directional          0.015, 0.001   [0.015, 0.001]
    sizes, specular_directional (k = 6) 0.076, 0.010   [0.084, 0.011]
    sizes, diffuse_point                0.015, 0.002   [0.017, 0.002]
    kinks                               0.004, 0.002   [0.004, 0.001]
    back-facing, one-sided              0.037, 0.005   [0.037, 0.007]
    shininess 0 .. 50, int and float    0.26,  0.046   [0.26,  0.049]   (both maxima at k = 50)
    position on the light               0.003, 0.004   [0.003, 0.004]
    non-finite rows                     0.043, 0.007   [0.033, 0.004]
    vertex_normals, single triangle     0.004, 0.000   [0.010, 0.001]
    vertex_normals, strips 255 .. 257   0.013, 0.001   [0.014, 0.002]
    vertex_normals, fan of valence 512  0.23,  0.007   [0.14,  0.010]   (7.7e-7 on a component that is 0)
    vertex_normals, unreferenced / degenerate / out of range   0.010, 0.001   [0.012, 0.002]
    vertex_normals, 70,000 frames       0.017, 0.001   [0.018, 0.002]
(`pytest -s` prints them per case.)
"""
import numpy as np
import pytest
import torch

import lighting_cases as lc
import lighting_f64
from dirt_amd import lighting

OPS = {"diffuse": lighting._diffuse_directional_ops, "specular": lighting._specular_directional_ops,
       "point": lighting._diffuse_point_ops}
FD_STEP, FD_PIN = 1e-6, 1e-6
F64_PIN = 1e-12
THIRD = 1.0 / 3.0


# ---- the statement against central differences

def _fd(f, xs, g, h=FD_STEP):
    """central differences of sum(f(*xs) * g) with respect to every element of every array in xs"""
    out = []
    for i, x in enumerate(xs):
        d = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            hi, lo = [y.copy() for y in xs], [y.copy() for y in xs]
            hi[i][idx] += h
            lo[i][idx] -= h
            d[idx] = ((f(*hi) - f(*lo)) * g).sum() / (2 * h)
        out.append(d)
    return out


def _fd_check(name, fd, vjp):
    worst = 0.0
    for a, b in zip(fd, vjp):
        scale = max(np.abs(a).max(), np.abs(b).max(), 1e-30)
        worst = max(worst, np.abs(a - b).max() / scale)
    print("%s: central differences within %.3g of the scale" % (name, worst))
    assert worst <= FD_PIN, "%s: %.3g of the scale" % (name, worst)


def _smooth_rows(fn, two, n=6):
    """rows of a random case well away from the kink (|cos| > 0.2)"""
    big = lc.random_case(fn, (200, 3), two, seed=21)
    keep = np.flatnonzero(np.abs(lc._cos(fn, big.operands, big.params)) > 0.2)[:n]
    return [x[keep].astype(np.float64) for x in big.operands], [p.astype(np.float64) for p in big.params], \
        big.grad[keep].astype(np.float64)


@pytest.mark.parametrize("two", [True, False])
def test_statement_diffuse_directional_vjp(two):
    ops, params, g = _smooth_rows("diffuse", two)
    v = lighting_f64.diffuse_directional_vjp(*ops, *params, two, g)
    fd = _fd(lambda *a: lighting_f64.diffuse_directional(*a, two), ops + params, g)
    _fd_check("diffuse_directional", fd, [v[k] for k in lc.OPERANDS["diffuse"] + lc.PARAMS["diffuse"]])


@pytest.mark.parametrize("two,k", [(True, 6.0), (False, 2.5), (True, 0.5), (False, 1.0)])
def test_statement_specular_directional_vjp(two, k):
    ops, params, g = _smooth_rows("specular", two)
    if not two:  # one-sided: front-facing rows only (behind the clamp everything is identically 0)
        ops2, params, g2 = _smooth_rows("specular", True, n=40)
        front = lc._cos("specular", ops2, params) > 0.2
        ops, g = [x[front][:6] for x in ops2], g2[front][:6]
    xs = ops + params + [np.array(k)]
    v = lighting_f64.specular_directional_vjp(*ops, *params, k, two, g)
    fd = _fd(lambda *a: lighting_f64.specular_directional(*a[:-1], float(a[-1]), two), xs, g)
    names = lc.OPERANDS["specular"] + lc.PARAMS["specular"] + ("shininess",)
    _fd_check("specular_directional", fd, [np.asarray(v[n]) for n in names])


@pytest.mark.parametrize("two", [True, False])
def test_statement_diffuse_point_vjp(two):
    ops, params, g = _smooth_rows("point", two)
    v = lighting_f64.diffuse_point_vjp(*ops, *params, two, g)
    fd = _fd(lambda *a: lighting_f64.diffuse_point(*a, two), ops + params, g)
    _fd_check("diffuse_point", fd, [v[k] for k in lc.OPERANDS["point"] + lc.PARAMS["point"]])


@pytest.mark.parametrize("layout", ["v3", "v4", "b3"])
def test_statement_vertex_normals_vjp(layout):
    mesh = lc.grid_mesh()
    x, g = mesh.vertices(layout).astype(np.float64), mesh.grad(layout).astype(np.float64)
    fd, = _fd(lambda v: lighting_f64.vertex_normals(v, mesh.faces), [x], g)
    vjp = lighting_f64.vertex_normals_vjp(x, mesh.faces, g)
    if layout == "v4":
        assert np.all(vjp[:, 3] == 0) and np.all(fd[:, 3] == 0)
    _fd_check("vertex_normals", [fd], [vjp])


def test_statement_drops_out_of_range_faces():
    mesh = lc.grid_mesh()
    x, g = mesh.vertices("b3"), mesh.grad("b3")
    for dtype in (np.int32, np.int64):
        mixed, good = lc.out_of_range_faces(dtype)
        assert len(mixed) > len(good)
        np.testing.assert_array_equal(lighting_f64.vertex_normals(x, mixed), lighting_f64.vertex_normals(x, good))
        np.testing.assert_array_equal(lighting_f64.vertex_normals_vjp(x, mixed, g),
                                      lighting_f64.vertex_normals_vjp(x, good, g))


def test_statement_kink_conventions():
    """The conventions the docstring of lighting_f64 states, each at a point built for it."""
    one = np.ones((1, 3))
    ld, lcol = np.array([0.0, 1.0, 0.0]), np.ones(3)
    n = np.array([[1.0, 0.0, 0.0]])  # cos = 0 exactly
    for two in (True, False):
        v = lighting_f64.diffuse_directional_vjp(n, one, ld, lcol, two, one)
        np.testing.assert_array_equal(v["normals"], 0 * n if two else 3.0 * -ld[None])  # sign(0) = 0; x >= 0 passes
    nan = np.array([[np.nan, 0.0, 0.0]])
    for two in (True, False):
        assert np.isnan(lighting_f64.diffuse_directional(nan, one, ld, lcol, two)).all()
        v = lighting_f64.diffuse_directional_vjp(nan, one, ld, lcol, two, one)
        np.testing.assert_array_equal(v["normals"], 0 * n)
    # a back-facing one-sided point under k = 0.5: k x^(k-1) is infinite at 0, the select gives exactly 0
    back = lighting_f64.specular_directional_vjp(np.array([[0.0, 0.0, 1.0]]),np.array([[0.0, 0.0, 1.0]]), one,
                                                 np.array([0.0, 0.0, -1.0]), lcol, np.zeros(3), 0.5, False, one)
    for k in ("positions", "normals", "reflectivities"):
        np.testing.assert_array_equal(back[k], np.zeros((1, 3)))
    # a position on the light: |0| has gradient 0, so the double-sided gradient is 0 and the one-sided is n g / eps
    p = lighting_f64.diffuse_point_vjp(np.zeros((1, 3)), n, one, np.zeros(3), lcol, False, one)
    np.testing.assert_allclose(p["positions"], 3.0 * n / 1e-12, rtol=1e-12)
    p = lighting_f64.diffuse_point_vjp(np.zeros((1, 3)), n, one, np.zeros(3), lcol, True, one)
    assert np.all(p["positions"] == 0)


# ---- the framework-op statement against the float64 statement, on the shared table

def _run_ops(case, dtype, light_grads):
    ops = [torch.from_numpy(x).to(dtype).requires_grad_(True) for x in case.operands]
    params = [torch.from_numpy(p).to(dtype).requires_grad_(light_grads) for p in case.params]
    args = ops + params
    if case.fn == "specular":
        k = case.shininess
        if light_grads:  # a tensor exponent takes the framework path too; its gradient is pinned with the rest
            k = torch.tensor(float(k), dtype=dtype, requires_grad=True)
        args = args + [k]
    y = OPS[case.fn](*args, case.two)
    wrt = [a for a in args if isinstance(a, torch.Tensor) and a.requires_grad]
    grads = torch.autograd.grad(y, wrt, torch.from_numpy(case.grad).to(dtype))
    names = lc.OPERANDS[case.fn] + lc.PARAMS[case.fn] + ("shininess",)
    return y.detach().numpy(), {n: g.numpy() for n, g in zip(names, grads)}


def _ratios(case, y, grads, frac, big_rtol):
    """(forward, gradient) worst error over bound against the statement, for the gradients present"""
    ref_y, ref_g = case.reference()
    worst = 0.0
    colour = lc.OPERANDS[case.fn][-1]
    for name, g in grads.items():
        per_row = name in lc.OPERANDS[case.fn]
        rows = case.rows if per_row and name != colour else None
        big = case.big_rows if name == "positions" else ()
        worst = max(worst, lc.grad_ratio(g, np.asarray(ref_g[name]), "%s d %s" % (case.id, name), rows, big,
                                         frac=frac, big_rtol=big_rtol))
    return lc.fwd_ratio(y, ref_y, case.id), worst


CASES = lc.elementwise_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_ops_float64_match_statement(case):
    y, grads = _run_ops(case, torch.float64, light_grads=case.rows is None)  # (light sums: finite rows only)
    ref_y, ref_g = case.reference()
    _, ref_y64, fin = lc._same_nonfinite(y, ref_y, case.id)
    scale = max(np.abs(ref_y64[fin]).max(initial=0.0), 1e-30)
    with np.errstate(invalid="ignore"):
        assert np.abs(y - ref_y64)[fin].max(initial=0.0) <= F64_PIN * scale
    _, worst = _ratios(case, y, grads, frac=F64_PIN, big_rtol=F64_PIN)
    print("%s: float64 gradients within %.3g of scale" % (case.id, worst * F64_PIN))
    assert worst <= 1.0, "%s: gradients %.3g x 1e-12 of scale" % (case.id, worst)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_ops_float32_within_a_third_of_the_contract(case):
    y, grads = _run_ops(case, torch.float32, light_grads=False)
    fwd, grad = _ratios(case, y, grads, frac=lc.GRAD_FRAC, big_rtol=lc.BIG_ROW_RTOL)
    print("%s: forward %.3f, gradients %.3f of the contract" % (case.id, fwd, grad))
    assert fwd <= THIRD and grad <= THIRD, "%s: forward %.3f, gradients %.3f of the contract" % (case.id, fwd, grad)


MESHES = lc.mesh_cases()


def _vn_ops(x, faces, g, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = lighting._vertex_normals_ops(xt, torch.from_numpy(np.asarray(faces, np.int64)))
    gx, = torch.autograd.grad(y, [xt], torch.from_numpy(g).to(dtype))
    return y.detach().numpy(), gx.numpy()


def _vn_check(ident, x, faces, g, zero_rows=None):
    ref_y, ref_g = lighting_f64.vertex_normals(x, faces), lighting_f64.vertex_normals_vjp(x, faces, g)
    y, gx = _vn_ops(x, faces, g, torch.float64)
    assert np.abs(y - ref_y).max(initial=0.0) <= F64_PIN
    worst = lc.grad_ratio(gx, ref_g, ident + " d vertices (float64)", frac=F64_PIN)
    print("%s: float64 gradients within %.3g of scale" % (ident, worst * F64_PIN))
    assert worst <= 1.0
    y, gx = _vn_ops(x, faces, g, torch.float32)
    fwd, grad = lc.fwd_ratio(y, ref_y, ident), lc.grad_ratio(gx, ref_g, ident + " d vertices")
    print("%s: forward %.3f (max err %.3g), gradients %.3f of the contract" % (
        ident, fwd, np.abs(y - ref_y).max(initial=0.0), grad))
    assert fwd <= THIRD and grad <= THIRD, "%s: forward %.3f, gradients %.3f of the contract" % (ident, fwd, grad)
    return y, gx


@pytest.mark.parametrize("layout", ["v3", "v4", "b3"])
@pytest.mark.parametrize("mesh", MESHES, ids=[m.id for m in MESHES])
def test_vertex_normals_ops_match_statement(mesh, layout):
    x, g = mesh.vertices(layout), mesh.grad(layout)
    y, gx = _vn_check("%s-%s" % (mesh.id, layout), x, mesh.faces, g)
    if "unreferenced" in mesh.marks:
        rows = list(mesh.marks["unreferenced"])
        assert np.all(y[..., rows, :] == 0) and np.all(gx[..., rows, :] == 0)
        only = np.zeros_like(g)
        only[..., rows, :] = g[..., rows, :]
        assert np.all(lighting_f64.vertex_normals_vjp(x, mesh.faces, only) == 0)
        assert np.all(_vn_ops(x, mesh.faces, only, torch.float32)[1] == 0)
    assert np.isfinite(gx).all()


def test_vertex_normals_ops_empty_and_many_frames():
    x = lc.grid_mesh().vertices("v3")
    none = np.zeros((0, 3), np.int64)
    y, gx = _vn_ops(x, none, np.ones_like(x), torch.float32)
    assert np.all(y == 0) and np.all(gx == 0)
    assert np.all(lighting_f64.vertex_normals(x, none) == 0)
    assert np.all(lighting_f64.vertex_normals_vjp(x, none, x) == 0)
    assert lighting_f64.vertex_normals(np.zeros((0, 3), np.float32), none).shape == (0, 3)
    xs, g = lc.many_frames()
    _vn_check("many-frames", xs, [[0, 1, 2]], g)
