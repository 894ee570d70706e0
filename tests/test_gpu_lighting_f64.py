"""Fused lighting kernels (dirt_amd/csrc/lighting_kernels.h) against the float64 statement of the reference's
formulas (tests/lighting_f64.py) at edge shapes, under the project's float32 contract (tests/test_gpu_lighting.py):
forward within 2e-6 + 1e-5 |ref|, gradients within 1e-4 of the gradient's scale.  The framework-op statement in
float32 on a CPU stays within a third of that contract on every case here (tests/test_lighting_f64.py, which lists
the measured margins), so a failure is the kernel's.

Every comparison is NaN-safe (lighting_cases.fwd_ratio / grad_ratio): the non-finite patterns must agree, and a NaN
where the statement is finite fails.  The fused node must be the one that ran (grad_fn of the C++ autograd
functions), except in the dispatch test, where it must not.

vertex_normals, degenerate faces: the backward is asserted only with a zero upstream gradient on the vertices such
faces touch.  With a non-zero one the face's dn / 1e-12 terms, of order 1e12, cancel against each other through the
scatter's atomics -- in any implementation and any precision the result is rounding noise of that magnitude.

Measured on an MI355X: 203 cases in 4 s; every case within 0.26 of the forward bound and 0.05 of the gradient
bound (tests/test_lighting_f64.py lists them per group).  The 70,000-frame launch (grid y extent = frames) runs as
it is.  The one-sided non-finite cases failed before shade_clamp became a compare-select ("NaN pattern differs
(0 vs 6 in the statement)": fmaxf(NaN, 0) = 0).
"""
import itertools

import numpy as np
import pytest
import torch

import lighting_cases as lc
import lighting_f64
from dirt_amd import lighting

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FUSED = {"diffuse": (lighting.diffuse_directional, "DiffuseFn"),
         "specular": (lighting.specular_directional, "SpecularFn"),
         "point": (lighting.diffuse_point, "DiffusePointFn")}


def _fused_node(y, cls):
    assert y.grad_fn is not None and cls in y.grad_fn.name(), y.grad_fn.name() if y.grad_fn else None


def _gpu(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(grad)


def _run(case, operands=None):
    """The public call on the GPU -> (forward, {operand name: gradient}); `operands` replaces the case's own
    leaf tensors (any layout)."""
    fn, node = FUSED[case.fn]
    ops = operands or [_gpu(x, True) for x in case.operands]
    args = ops + [_gpu(p) for p in case.params] + ([case.shininess] if case.fn == "specular" else [])
    y = fn(*args, double_sided=case.two)
    _fused_node(y, node)
    wrt = [(n, x) for n, x in zip(lc.OPERANDS[case.fn], ops) if x.requires_grad]
    grads = torch.autograd.grad(y, [x for _, x in wrt], _gpu(case.grad))
    return y.detach().cpu().numpy(), {n: g.cpu().numpy() for (n, _), g in zip(wrt, grads)}


def _check(case, y, grads):
    """forward and the gradients present within the contract of the float64 statement"""
    ref_y, ref_g = case.reference()
    r = lc.fwd_ratio(y, ref_y, case.id)
    print("%s: forward at %.3f of the contract" % (case.id, r))
    assert r <= 1.0, "%s: forward at %.3g of the contract" % (case.id, r)
    colour = lc.OPERANDS[case.fn][-1]
    for name, g in grads.items():
        assert g.dtype == np.float32
        r = lc.grad_ratio(g, ref_g[name], "%s d %s" % (case.id, name), None if name == colour else case.rows,
                          case.big_rows if name == "positions" else ())
        print("%s: d %s at %.3f of the contract" % (case.id, name, r))
        assert r <= 1.0, "%s: d %s at %.3g of the contract" % (case.id, name, r)


def _check_exact(case, y, grads):
    """what must hold exactly, by the statement's conventions at the kinks"""
    geometry = [grads[n] for n in lc.OPERANDS[case.fn][:-1]]
    if "kink" in case.marks:
        rows = case.marks["kink"]
        assert np.all(y[rows] == 0), "forward is not exactly 0 at the kink"
        if case.two:  # d|x| at 0 is 0; one-sided the gradient passes (x >= 0), which _check holds to the statement
            assert all(np.all(g[rows] == 0) for g in geometry)
        elif case.shininess in (None, 1.0):  # (x^2 has slope 0 there)
            assert any(np.any(g[rows] != 0) for g in geometry)
    if "back" in case.marks and not case.two:
        rows = case.marks["back"]
        if case.shininess not in (0, 0.0):  # (0^0 = 1: a zero exponent lights back-facing points too)
            assert np.all(y[rows] == 0), "a back-facing one-sided point is lit"
            assert all(np.all(g[rows] == 0) for g in grads.values()), "a back-facing one-sided point has a gradient"
        assert np.isfinite(y).all() and all(np.isfinite(g).all() for g in grads.values())
    if case.fn == "specular" and case.shininess in (0, 0.0) and case.rows is None:
        assert all(np.all(g == 0) for g in geometry), "x^0 has a gradient"
    for b in case.big_rows:
        assert np.all(y[b] == 0)


CASES = lc.elementwise_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_elementwise_kernels_match_statement(case):
    """Sizes around the wave and block edges, [H, W, 3] forms, kinks, back-facing rows, every shininess, a position
    on the light, non-finite rows (lighting_cases.elementwise_cases)."""
    y, grads = _run(case)
    assert y.shape == case.operands[0].shape
    _check(case, y, grads)
    _check_exact(case, y, grads)


def _subsets(fn):
    names = lc.OPERANDS[fn]
    return [(fn, s) for r in range(1, len(names) + 1) for s in itertools.combinations(names, r)]


@pytest.mark.parametrize("fn,subset", [x for fn in lc.OPERANDS for x in _subsets(fn)],
                         ids=lambda v: v if isinstance(v, str) else "+".join(v))
@pytest.mark.parametrize("two", [True, False])
def test_gradient_subsets(fn, subset, two):
    """Every non-empty subset of operands requiring a gradient: the kernels' null-pointer branches."""
    case = lc.random_case(fn, (65, 3), two, seed=31)
    ops = [_gpu(x, n in subset) for n, x in zip(lc.OPERANDS[fn], case.operands)]
    y, grads = _run(case, ops)
    assert tuple(grads) == subset
    _check(case, y, grads)
    # and through backward(): nothing arrives where nothing was asked for
    ops = [_gpu(x, n in subset) for n, x in zip(lc.OPERANDS[fn], case.operands)]
    args = ops + [_gpu(p) for p in case.params] + ([case.shininess] if fn == "specular" else [])
    FUSED[fn][0](*args, double_sided=two).backward(_gpu(case.grad))
    for n, x in zip(lc.OPERANDS[fn], ops):
        assert (x.grad is not None) == (n in subset)
        if n in subset:
            np.testing.assert_array_equal(x.grad.cpu().numpy(), grads[n])


@pytest.mark.parametrize("form", ["transposed", "sliced", "expanded"])
@pytest.mark.parametrize("fn", list(lc.OPERANDS))
def test_noncontiguous_operands(fn, form):
    """Views as operands: the gradients arrive in the layout of the leaf tensor."""
    case = lc.random_case(fn, (65, 3), True, seed=32)
    ref_y, ref_g = case.reference()
    names = lc.OPERANDS[fn]
    if form == "transposed":
        leaves = [_gpu(x.T, True) for x in case.operands]  # [3, N] leaves
        ops = [x.t() for x in leaves]
        expect = [np.asarray(ref_g[n]).T for n in names]
    elif form == "sliced":
        rng = np.random.default_rng(33)
        padded = []
        for x in case.operands:
            p = rng.standard_normal((130, 3)).astype(np.float32)
            p[::2] = x
            padded.append(p)
        leaves = [_gpu(p, True) for p in padded]
        ops = [x[::2] for x in leaves]
        expect = []
        for n in names:
            e = np.zeros((130, 3))
            e[::2] = ref_g[n]
            expect.append(e)
    else:  # one [1, 3] colour for every row, materialised before the call
        case.operands[-1][:] = case.operands[-1][:1]
        del case._ref
        ref_y, ref_g = case.reference()
        leaves = [_gpu(x, True) for x in case.operands[:-1]] + [_gpu(case.operands[-1][:1], True)]
        ops = leaves[:-1] + [leaves[-1].expand(65, 3).contiguous()]
        expect = [np.asarray(ref_g[n]) for n in names[:-1]] + [np.asarray(ref_g[names[-1]]).sum(0, keepdims=True)]
    assert form == "expanded" or not any(x.is_contiguous() for x in ops)
    fn_, node = FUSED[fn]
    args = ops + [_gpu(p) for p in case.params] + ([case.shininess] if fn == "specular" else [])
    y = fn_(*args, double_sided=True)
    _fused_node(y, node)
    assert lc.fwd_ratio(y.detach().cpu().numpy(), ref_y, case.id) <= 1.0
    y.backward(_gpu(case.grad))
    for n, leaf, e in zip(names, leaves, expect):
        assert leaf.grad.shape == leaf.shape
        r = lc.grad_ratio(leaf.grad.cpu().numpy(), e, "%s %s d %s" % (fn, form, n))
        assert r <= 1.0, "%s %s: d %s at %.3g of the contract" % (fn, form, n, r)


def test_routed_inputs_meet_the_statement_without_a_fused_node():
    """What lighting.py routes to the framework ops -- float64 operands, a broadcast [1, 3] colour, a tensor
    shininess, a light that needs a gradient -- meets the same statement on the GPU, with no fused node."""
    routes = [(f, r) for f in lc.OPERANDS for r in ("float64", "broadcast", "light_grad")] + [("specular", "tensor_k")]
    for fn, route in routes:
        case = lc.random_case(fn, (65, 3), True, seed=34)
        call, node = FUSED[fn]
        names = lc.OPERANDS[fn]
        if route == "broadcast":
            case.operands[-1][:] = case.operands[-1][:1]
        ref_y, ref_g = case.reference()
        dt = torch.float64 if route == "float64" else torch.float32
        ops = [_gpu(x).to(dt).requires_grad_(True) for x in case.operands]
        if route == "broadcast":
            ops[-1] = _gpu(case.operands[-1][:1], True)
        params = [_gpu(p).to(dt).requires_grad_(route == "light_grad" and i == 0) for i, p in enumerate(case.params)]
        k = [] if fn != "specular" else [case.shininess]
        if route == "tensor_k":
            k = [torch.tensor(case.shininess, device=DEV)]
        y = call(*ops, *params, *k, double_sided=True)
        assert node not in y.grad_fn.name(), "%s %s ran the fused kernel" % (fn, route)
        what = "%s routed by %s" % (fn, route)
        assert lc.fwd_ratio(y.detach().cpu().numpy(), ref_y, what) <= 1.0, what
        wrt = ops + params[:1] if route == "light_grad" else ops
        grads = torch.autograd.grad(y, wrt, _gpu(case.grad).to(dt))
        expect = [np.asarray(ref_g[n]) for n in names]
        if route == "broadcast":
            expect[-1] = expect[-1].sum(0, keepdims=True)
        if route == "light_grad":
            expect.append(np.asarray(ref_g[lc.PARAMS[fn][0]]))
        for g, e in zip(grads, expect):
            assert lc.grad_ratio(g.cpu().numpy(), e, what) <= 1.0, what


# ---- vertex_normals

def _vn(x, faces, g, want_grad=True):
    xt = _gpu(x, True)
    y = lighting.vertex_normals(xt, torch.from_numpy(np.ascontiguousarray(faces)).to(DEV))
    _fused_node(y, "VertexNormalsFn")
    gx, = torch.autograd.grad(y, [xt], _gpu(g))
    assert gx.shape == xt.shape and y.shape == xt.shape[:-1] + (3,)
    return y.detach().cpu().numpy(), gx.cpu().numpy()


def _vn_check(ident, y, gx, x, faces, g):
    ref_y, ref_g = lighting_f64.vertex_normals(x, faces), lighting_f64.vertex_normals_vjp(x, faces, g)
    r = lc.fwd_ratio(y, ref_y, ident)
    print("%s: forward at %.3f of the contract" % (ident, r))
    assert r <= 1.0, "%s: forward at %.3g of the contract" % (ident, r)
    r = lc.grad_ratio(gx, ref_g, ident + " d vertices")
    print("%s: d vertices at %.3f of the contract" % (ident, r))
    assert r <= 1.0, "%s: d vertices at %.3g of the contract" % (ident, r)


MESHES = lc.mesh_cases()


@pytest.mark.parametrize("layout", ["v3", "v4", "b3"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("mesh", MESHES, ids=[m.id for m in MESHES])
def test_vertex_normals_meshes(mesh, dtype, layout):
    """One triangle; strips whose face count straddles the block; a 512-valence hub (two workgroups of atomics on
    one vertex); unreferenced vertices; degenerate faces."""
    x, g, faces = mesh.vertices(layout), mesh.grad(layout), mesh.faces.astype(dtype)
    y, gx = _vn(x, faces, g)
    _vn_check("%s-%s" % (mesh.id, layout), y, gx, x, faces, g)
    assert np.isfinite(gx).all()
    if layout == "v4":
        assert np.all(gx[:, 3] == 0)
    if "unreferenced" in mesh.marks:
        rows = list(mesh.marks["unreferenced"])
        assert np.all(y[..., rows, :] == 0) and np.all(gx[..., rows, :] == 0)
        only = np.zeros_like(g)
        only[..., rows, :] = g[..., rows, :]
        assert np.all(_vn(x, faces, only)[1] == 0), "a gradient on an unreferenced vertex reached another vertex"


@pytest.mark.parametrize("layout", ["v3", "v4", "b3"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
def test_vertex_normals_skips_out_of_range_faces(dtype, layout):
    """-1, V and 2^31 - 1 (and 2^40 as int64): forward and backward equal the statement with those faces removed."""
    mesh = lc.grid_mesh()
    x, g = mesh.vertices(layout), mesh.grad(layout)
    mixed, good = lc.out_of_range_faces(dtype)
    y, gx = _vn(x, mixed, g)
    _vn_check("out-of-range-%s" % layout, y, gx, x, good, g)


def test_vertex_normals_empty_meshes():
    x = lc.grid_mesh().vertices("v3")
    none = np.zeros((0, 3), np.int32)
    y, gx = _vn(x, none, np.ones_like(x))
    assert np.all(y == 0) and np.all(gx == 0)
    for faces in (none, np.array([[0, 1, 2]], np.int64)):
        y, gx = _vn(np.zeros((0, 3), np.float32), faces, np.zeros((0, 3), np.float32))
        assert y.shape == (0, 3) and gx.shape == (0, 3)
        y, gx = _vn(np.zeros((2, 0, 4), np.float32), faces, np.zeros((2, 0, 3), np.float32))
        assert y.shape == (2, 0, 3) and gx.shape == (2, 0, 4)


def test_vertex_normals_many_frames():
    """70,000 frames of one face: more than the 65,535 a grid's y extent is specified to hold."""
    x, g = lc.many_frames()
    faces = np.array([[0, 1, 2]], np.int32)
    y, gx = _vn(x, faces, g)
    _vn_check("many-frames", y, gx, x, faces, g)
