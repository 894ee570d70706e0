"""The fused shadow-map lookup (dirt_amd/csrc/shadow_kernels.h through dirt_amd.deferred.sample_shadow) against the
numpy statement of record (tests/shadow_cases.py) on its whole table.

Forward and valid: bit-exact against the float32 statement; unsampled pixels exactly 0, sampled pixels that are not
inside the light's frustum exactly 1.
The float64 statement of the gradients starts from what the float32 forward rounded (taps, weights, s values, pass
flags, cx, cy, 1 / cw, 1 / softness), so only the backward's own float32 operations separate the kernels from it; the
bounds count them on the longest path, in units of 2^-24 times the sum of the absolute terms (shadow_kernels.h's
header has the order of the operations, shadow_cases.py the sums):
  the adjoint of the clip coordinates: g_cz passes 5 roundings (the sum inside mt, mt * omb, the sum of the two
    products, the product with g, the product with 1 / softness); g_cx and g_cy 6 (the difference of two s values --
    or the product and the sum inside top / bot --, the product with the weight, the sum of the two products, the
    product with g, the product with Sw or Sh, the product with 1 / cw; the halving is exact); g_cw 9 (the 5 of g_u,
    nx * cx, the sum nx * cx + ny * cy, two products with 1 / cw): at most 9.
  grad_positions: each of its four terms one more product, then at most three additions, each rounding a partial sum
    of at most the sum of the absolute terms, one unit for the second order: k = 9 + 1 + 3 + 1 = 14.
  grad_light_matrix: a term p_r * g_c[j] is 9 + 1 roundings; the n terms of the pixels inside the frustum are summed
    by n - 1 additions in the kernels' fixed grouping (lanes, waves, tiles, frames; the other pixels add exact zeros),
    each rounding a partial sum of at most the sum S of the absolute terms; the n-th unit absorbs the second order:
    (n + 10) * 2^-24 * S.
  grad_depth_map: a term ((g * wa) * wb) * (1 / softness) is three float32 products; n terms are summed by n - 1
    additions in whatever order the atomics arrive and however they are grouped (LDS patch first or not):
    (n + 3) * 2^-24 * S, as texture_cases.texture_bound.
grad_positions and grad_light_matrix are bit-identical between two runs (no atomics on their path).
Each test prints its worst measured ratio of error to bound (on an MI355X, over the table: grad_depth_map 0.571,
grad_positions 0.298, grad_light_matrix 0.085).
"""
import gc

import numpy as np
import pytest
import torch

import deferred_pipeline as dp
import shadow_cases as sc
from dirt_amd import deferred

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAMES = ("grad_depth", "grad_positions", "grad_matrix")
BOUNDS = {"grad_depth": sc.depth_bound, "grad_positions": sc.positions_bound, "grad_matrix": sc.matrix_bound}


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fused_node(y, cls="_SampleShadowFn"):
    """y comes from the fused autograd function `cls` (directly, or through the [0] of an unbatched call)"""
    assert y.grad_fn is not None
    names = [y.grad_fn.name()] + [fn.name() for fn, _ in y.grad_fn.next_functions if fn is not None]
    assert any(cls in n for n in names), names


def _run(inputs, needs=(True, True, True)):
    """-> (visibility [B,H,W], valid [B,H,W], grad_depth, grad_positions, grad_matrix or None each) as numpy"""
    depth, pos, M, bias, softness, mask, grad = inputs
    ts = [_gpu(a).requires_grad_(need) for a, need in zip((depth, pos, M), needs)]
    vis, valid = deferred.sample_shadow(*ts, bias, softness, _gpu(mask))
    assert not valid.requires_grad and valid.dtype == torch.bool and vis.shape == valid.shape == pos.shape[:-1] + (1,)
    if any(needs):
        _fused_node(vis)
        vis.backward(_gpu(grad)[..., None])
    else:
        assert not vis.requires_grad
    torch.cuda.synchronize()
    return (vis.detach().cpu().numpy()[..., 0], valid.cpu().numpy()[..., 0]) + tuple(
        None if t.grad is None else t.grad.cpu().numpy() for t in ts)


def _ratio(err, bound, tag):
    """worst err / bound; where the bound is 0 the error must be"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    zero = bound == 0
    assert not np.any(err[zero]), tag
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _check_forward(got, fwd, tag):
    vis, valid = got[0], got[1]
    assert np.array_equal(valid, fwd["valid"]), tag
    assert np.array_equal(_bits(vis), _bits(fwd["visibility"])), tag
    assert not np.any(_bits(vis)[~fwd["valid"]]), tag
    assert np.all(vis[fwd["valid"] & ~fwd["inside"]] == 1.0), tag


def _check_grads(got, vjp, tag):
    """-> {name: worst ratio of error to bound} of the gradients present"""
    ratios = {}
    for name, g in zip(NAMES, got[2:]):
        if g is None:
            continue
        assert g.shape == vjp[name].shape, (tag, name)
        ratios[name] = _ratio(np.abs(g - vjp[name]), BOUNDS[name](vjp), (tag, name))
        assert ratios[name] <= 1.0, (tag, name, ratios[name])
    return ratios


def _fmt(ratios):
    return ", ".join("%s %.3f" % (k, v) for k, v in ratios.items()) + " of the bound"


@pytest.mark.parametrize("ident", sc.CASE_IDS)
def test_matches_the_statement(ident):
    inputs, fwd, vjp = sc.case(ident)
    first, second = _run(inputs), _run(inputs)
    _check_forward(first, fwd, ident)
    for k in (3, 4):  # grad_positions, grad_light_matrix: no run-to-run difference
        assert np.array_equal(_bits(first[k]), _bits(second[k])), (ident, NAMES[k - 2])
    assert not np.any(_bits(first[3])[~fwd["inside"]]), ident
    if inputs[4] == 0:
        assert not np.any(first[2]), ident  # (no ramp: the depth map's gradient is the call's zero-fill)
    r1, r2 = _check_grads(first, vjp, ident), _check_grads(second, vjp, ident)
    r1["grad_depth"] = max(r1["grad_depth"], r2["grad_depth"])
    print("shadow %s: %s" % (ident, _fmt(r1)))


@pytest.mark.parametrize("kind,frames", [("magnify16", 1), ("scatter", 1), ("magnify16", 2), ("scatter", 2)])
def test_exact_scatter(kind, frames):
    """Weights in {0, 1/4, 1/2, 1}, 1 / softness = 4, depths and positions in eighths and small integer cotangents:
    every partial sum is exact in float32, so grad_depth equals the statement exactly whatever the order of the
    atomics -- through the LDS patch and its flush (magnify16), through the direct atomics (scatter), and summed over
    the frames of a shared map."""
    inputs, fwd, vjp = sc.exact_scatter_case(kind, frames)
    got = _run(inputs)
    _check_forward(got, fwd, kind)
    assert np.array_equal(got[2].astype(np.float64), vjp["grad_depth"]), kind
    assert np.count_nonzero(vjp["grad_depth"]) > 0 and not np.any(got[2][~np.isfinite(inputs[0])])
    _check_grads(got, vjp, kind)


SUBSET_IDENT = "2x33x18-m5x7-sP-ortho-soft-bias-random-bg"


@pytest.mark.parametrize("needs", [(False, False, False), (True, False, False), (False, True, False),
                                   (False, False, True)], ids=["none", "depth", "positions", "matrix"])
def test_gradient_subsets(needs):
    """Each gradient alone, and none: the requested one as in the run of all three (bit for bit but for the depth
    map's, which is held to its bound), the others None."""
    inputs, fwd, vjp = sc.case(SUBSET_IDENT)
    got, full = _run(inputs, needs), _run(inputs)
    _check_forward(got, fwd, SUBSET_IDENT)
    assert tuple(g is not None for g in got[2:]) == needs
    _check_grads(got, vjp, "subset %s" % (needs,))
    for k in (3, 4):
        if needs[k - 2]:
            assert np.array_equal(_bits(got[k]), _bits(full[k]))


def test_positions_gradient_does_not_depend_on_the_matrix_sums():
    inputs, _, _ = sc.case(SUBSET_IDENT)
    without, with_sums = _run(inputs, (True, True, False)), _run(inputs, (True, True, True))
    assert without[4] is None and with_sums[4] is not None
    assert np.array_equal(_bits(without[3]), _bits(with_sums[3])) and np.count_nonzero(without[3]) > 100


def test_forms(monkeypatch):
    """[H,W,3] positions with a shared map and matrix, non-contiguous views, bool and integer masks run the fused
    kernels; float64 and DIRT_FUSED_DEFERRED=0 take the statement, with no fused node."""
    ident = "15x17-m5x7-ss-ortho-soft-bias-random-mask"
    (depth, pos, M, bias, softness, mask, grad), fwd, vjp = sc.case(ident)
    assert mask is not None
    base = _run((depth, pos, M, bias, softness, mask, grad))
    _check_forward(base, fwd, ident)
    _check_grads(base, vjp, ident)
    # unbatched, bool mask
    ts = [_gpu(a).requires_grad_(True) for a in (depth, pos[0], M)]
    vis, valid = deferred.sample_shadow(*ts, bias, softness, _gpu(mask[0]).bool())
    _fused_node(vis)
    assert vis.shape == (15, 17, 1) and valid.shape == (15, 17, 1) and valid.dtype == torch.bool
    vis.backward(_gpu(grad[0])[..., None])
    assert np.array_equal(_bits(vis.detach().cpu().numpy()[..., 0]), _bits(base[0][0]))
    assert np.array_equal(_bits(ts[1].grad.cpu().numpy()), _bits(base[3][0]))
    assert np.array_equal(_bits(ts[2].grad.cpu().numpy()), _bits(base[4]))
    assert np.all(np.abs(ts[0].grad.cpu().numpy() - vjp["grad_depth"]) <= sc.depth_bound(vjp))
    # non-contiguous views, integer mask
    wide_d, wide_p = torch.zeros((5, 14, 1), device=DEV), torch.zeros((1, 15, 17, 6), device=DEV)
    wide_m = torch.zeros((4, 8), device=DEV)
    wide_d[:, ::2], wide_p[..., ::2], wide_m[:, ::2] = _gpu(depth), _gpu(pos), _gpu(M)
    for t in (wide_d, wide_p, wide_m):
        t.requires_grad_(True)
    assert not wide_d[:, ::2].is_contiguous() and not wide_m[:, ::2].is_contiguous()
    vis, valid = deferred.sample_shadow(wide_d[:, ::2], wide_p[..., ::2], wide_m[:, ::2], bias, softness,
                                        _gpu(mask).long())
    _fused_node(vis)
    vis.backward(_gpu(grad)[..., None])
    assert np.array_equal(_bits(vis.detach().cpu().numpy()[..., 0]), _bits(base[0]))
    assert np.array_equal(_bits(wide_p.grad.cpu().numpy()[..., ::2]), _bits(base[3]))
    assert np.array_equal(_bits(wide_m.grad.cpu().numpy()[:, ::2]), _bits(base[4]))
    assert float(wide_p.grad[..., 1::2].abs().max()) == 0.0 and float(wide_d.grad[:, 1::2].abs().max()) == 0.0
    assert np.all(np.abs(wide_d.grad.cpu().numpy()[:, ::2] - vjp["grad_depth"]) <= sc.depth_bound(vjp))
    # float64 and the switch: the framework-op statement
    f64 = sc.sample(depth, pos, M, bias, softness, mask, np.float64)
    d64 = _gpu(depth).double().requires_grad_(True)
    y64, v64 = deferred.sample_shadow(d64, _gpu(pos).double(), _gpu(M).double(), bias, softness, _gpu(mask))
    assert "_SampleShadowFn" not in y64.grad_fn.name()
    assert np.abs(y64.detach().cpu().numpy()[..., 0] - f64["visibility"]).max() <= 1e-12
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    dt = _gpu(depth).requires_grad_(True)
    y, v = deferred.sample_shadow(dt, _gpu(pos), _gpu(M), bias, softness, _gpu(mask))
    assert "_SampleShadowFn" not in y.grad_fn.name()
    assert np.array_equal(v.cpu().numpy()[..., 0], fwd["valid"])
    # (the framework ops do one IEEE operation per line too: the float32 statement bit for bit)
    assert np.array_equal(_bits(y.detach().cpu().numpy()[..., 0]), _bits(fwd["visibility"]))


def test_fused_backward_refuses_double_backward(monkeypatch):
    (depth, pos, M, bias, softness, mask, grad), _, _ = sc.case("15x17-m5x7-ss-ortho-soft-bias-random-mask")
    ts = [_gpu(a).requires_grad_(True) for a in (depth, pos, M)]
    vis, _ = deferred.sample_shadow(*ts, bias, softness, _gpu(mask))
    _fused_node(vis)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(vis.square().sum(), [ts[2]], create_graph=True)
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    vis, _ = deferred.sample_shadow(*ts, bias, softness, _gpu(mask))
    g, = torch.autograd.grad(vis.square().sum(), [ts[2]], create_graph=True)
    gg = torch.autograd.grad(g.square().sum(), ts[:2])
    assert all(bool(torch.isfinite(x).all()) for x in gg) and float(gg[0].abs().max()) > 0


def test_captures_into_a_graph():
    """One forward and backward captured with torch.cuda.graph on one stream (no parallel branches; the zero-fill of
    grad_depth is an asynchronous memset on it, the workspace comes from the graph's pool), replayed after the depth
    map, the positions and the matrix changed in place: equal to the eager result, bit for bit but for the depth
    map's gradient, which is held to its bound."""
    first = sc.case("63x65-m64x64-ss-ortho-soft-bias-magnify16-bg")[0]
    other = sc.case("63x65-m64x64-ss-ortho-soft-nobias-scatter")[0]
    bias, softness = first[3], first[4]  # (Python numbers: part of the captured launches)
    second = (other[0], other[1], other[2], bias, softness, None, other[6])
    fwd2 = sc.sample(*second[:6])
    vjp2 = sc.sample_vjp(second[0], second[1], second[2], second[6], fwd2)
    assert fwd2["inside"].mean() > 0.5 and np.count_nonzero(vjp2["grad_depth"]) > 1000
    ts = [_gpu(a).requires_grad_(True) for a in first[:3]]
    g = _gpu(second[6])[..., None]
    out = {}

    def step():
        vis, valid = deferred.sample_shadow(*ts, bias, softness)
        out["vis"], out["valid"] = vis, valid
        out["grads"] = torch.autograd.grad(vis, ts, g)

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
        for t, a in zip(ts, second[:3]):
            t.copy_(_gpu(a))
    graph.replay()
    torch.cuda.synchronize()
    got = (out["vis"].detach().cpu().numpy()[..., 0], out["valid"].cpu().numpy()[..., 0]) + tuple(
        x.cpu().numpy() for x in out["grads"])
    del graph
    out.clear()
    eager = _run(second)
    _check_forward(got, fwd2, "graph")
    assert np.array_equal(_bits(got[0]), _bits(eager[0])) and np.array_equal(got[1], eager[1])
    assert np.array_equal(_bits(got[3]), _bits(eager[3])) and np.array_equal(_bits(got[4]), _bits(eager[4]))
    print("graph replay: %s" % _fmt(_check_grads(got, vjp2, "graph")))


def chain_scene():
    """dp.grid_surface(n=12) plus a rectangular occluder patch 0.6 above it, and a light looking straight down from
    height 3: an orthographic box |x|, |z| <= 1.6, depths 0.5 to 6 -> (world, faces, albedo, light matrix)"""
    world, faces, albedo = dp.grid_surface(n=12)
    patch = np.array([[-0.5, 0.6, -0.4], [0.3, 0.6, -0.4], [0.3, 0.6, 0.4], [-0.5, 0.6, 0.4]], np.float32)
    n = len(world)
    world = np.concatenate([world, patch])
    faces = np.concatenate([faces, np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], np.int32)])
    albedo = np.concatenate([albedo, np.full((4, 3), 0.5, np.float32)])
    near, far, half = 0.5, 6.0, 1.6
    view = np.array([[1., 0., 0., 0.], [0., 0., 1., 0.], [0., -1., 0., 0.], [0., 0., -3., 1.]])
    proj = np.array([[1 / half, 0., 0., 0.], [0., 1 / half, 0., 0.], [0., 0., -2. / (far - near), 0.],
                     [0., 0., -(far + near) / (far - near), 1.]])
    return world, faces, albedo, (view @ proj).astype(np.float32)


CHAIN_MAP, CHAIN_BIAS, CHAIN_SOFTNESS = 48, 0.004, 0.03


def run_chain(lookup, render, device, H=64, W=64):
    """camera G-buffers -> the light's depth map (a 1-channel render of the light's clip z over +inf) -> `lookup` at
    the dilated positions -> one-light shade_lights times the visibility -> dp.loss_fn"""
    world, faces, albedo, ML = chain_scene()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    f, al = to(faces), to(albedo)
    wts = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(3)).to(device)
    Vw, M = to(world).requires_grad_(True), to(ML).requires_grad_(True)
    pos, col, nrm, _ = dp.gbuffers(render, Vw, f, al, H, W)
    clip_l = torch.cat([Vw, torch.ones_like(Vw[:, :1])], -1) @ M
    S = CHAIN_MAP
    depth = render(torch.full((S, S, 1), float("inf"), device=device), clip_l, clip_l[:, 2:3], f, S, S, 1)
    receivers = deferred.dilate(pos)
    vis, sampled = lookup(depth, receivers, M)
    lv = torch.tensor([[0., -1., 0.]], device=device)
    white = torch.ones((1, 3), device=device)
    pixels, valid = deferred.shade_lights(pos, col, nrm, lv, white, 0.5 * white, dp.camera_position(H, W, device), 6.)
    loss = dp.loss_fn(pixels * vis, valid & sampled, wts)
    g_vis, g_depth, g_m, g_v = torch.autograd.grad(loss, [vis, depth, M, Vw])
    return dict(vis=vis, sampled=sampled, valid=valid, receivers=receivers.detach(), depth=depth.detach(), M=M.detach(),
                g_vis=g_vis, g_depth=g_depth, g_m=g_m, g_v=g_v)


def test_chain_shadowed_deferred_shading():
    """The deferred chain at 64 x 64 with a shadowed light (run_chain).  The fused lookup against `_sample_shadow_ops`
    on the GPU, everything else shared: valid equal, the visibility bit for bit; d loss / d light_matrix and d loss /
    d depth_map within the statement's bounds for the fused path's own cotangent; d loss / d world vertices, which
    flows through the receivers' positions and through the occluder's depth render, within 1e-2 in relative L2 (the
    tolerance of test_chain_textured_deferred_shading for it).
    Measured on an MI355X: 34 % of the pixels lit, 2 % shadowed, 6.5 % on the ramp; d loss / d depth_map 0.485 of its
    bound, d loss / d light_matrix 0.001 of its bound through the lookup and 5.0e-7 in relative L2 from the framework
    ops' through the whole chain, d loss / d world vertices 3.6e-8 in relative L2."""
    fused = run_chain(lambda d, p, m: deferred.sample_shadow(d, p, m, CHAIN_BIAS, CHAIN_SOFTNESS), dp.hip_render, DEV)
    _fused_node(fused["vis"])
    ops = run_chain(lambda d, p, m: deferred._sample_shadow_ops(d, p, m, CHAIN_BIAS, CHAIN_SOFTNESS), dp.hip_render,
                    DEV)
    assert torch.equal(fused["sampled"], ops["sampled"]) and torch.equal(fused["valid"], ops["valid"])
    assert torch.equal(fused["depth"], ops["depth"]) and torch.equal(fused["receivers"], ops["receivers"])
    assert np.array_equal(_bits(fused["vis"].detach().cpu().numpy()), _bits(ops["vis"].detach().cpu().numpy()))
    depth, pos, M = (fused[k].cpu().numpy() for k in ("depth", "receivers", "M"))
    fwd = sc.sample(depth, pos[None], M, CHAIN_BIAS, CHAIN_SOFTNESS)
    assert np.array_equal(fwd["valid"][0], fused["sampled"].cpu().numpy()[..., 0])
    assert np.array_equal(_bits(fused["vis"].detach().cpu().numpy()[..., 0]), _bits(fwd["visibility"][0]))
    shares = sc.classes(fwd)
    assert shares["lit"] > 0.05 and shares["shadowed"] > 0.01 and shares["ramp"] > 0.01, shares
    vjp = sc.sample_vjp(depth, pos[None], M, fused["g_vis"].cpu().numpy()[None, ..., 0], fwd)
    r_depth = _ratio(np.abs(fused["g_depth"].cpu().numpy() - vjp["grad_depth"]), sc.depth_bound(vjp), "chain depth")
    # (the matrix also feeds the depth render: take the lookup's own share, d loss / d M through the lookup alone)
    m_leaf = fused["M"].clone().requires_grad_(True)
    vis, _ = deferred.sample_shadow(fused["depth"], fused["receivers"], m_leaf, CHAIN_BIAS, CHAIN_SOFTNESS)
    _fused_node(vis)
    g_m, = torch.autograd.grad(vis, [m_leaf], fused["g_vis"])
    r_m = _ratio(np.abs(g_m.cpu().numpy() - vjp["grad_matrix"]), sc.matrix_bound(vjp), "chain matrix")
    rel_l2 = float(torch.linalg.norm(fused["g_v"] - ops["g_v"]) / torch.linalg.norm(ops["g_v"]))
    rel_m = float(torch.linalg.norm(fused["g_m"] - ops["g_m"]) / torch.linalg.norm(ops["g_m"]))
    print("shadowed chain 64x64: classes %s; d loss / d depth_map %.3f of its bound, d loss / d light_matrix %.3f of "
          "its bound (whole chain: %.3g in relative L2 from the framework ops'), d loss / d world vertices rel L2 %.3g"
          % ({k: round(float(v), 3) for k, v in shares.items()}, r_depth, r_m, rel_m, rel_l2))
    assert r_depth <= 1.0 and r_m <= 1.0
    assert bool(torch.isfinite(fused["g_v"]).all()) and float(ops["g_v"].abs().max()) > 0
    n_surface = len(dp.grid_surface(n=12)[0])
    assert float(fused["g_v"][n_surface:].abs().max()) > 0 and float(fused["g_v"][:n_surface].abs().max()) > 0
    assert rel_l2 < 1e-2 and rel_m < 1e-2, (rel_l2, rel_m)
