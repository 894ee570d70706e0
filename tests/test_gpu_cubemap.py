"""The fused cube-map kernels (dirt_amd/csrc/cubemap_kernels.h through dirt_amd.deferred.sample_cubemap) against the
numpy statement of record (tests/cubemap_cases.py) on its whole table.

Forward and valid: bit-exact against the float32 statement, unsampled pixels exactly 0.
grad_directions: bit-identical between two runs (a gather in a fixed order), and within k * 2^-24 * (sum of the
absolute terms) of the float64 statement, k = C + 8 (cubemap_cases.directions_roundings: the C + 5 of a texture's uv
gradient, then a product, a sum and a division for the major axis' component; the other two take one division).
grad_cubemap: within (n + 2) * 2^-24 * S per element, the texture scatter's bound, whichever way a tile is summed (LDS
patch of one face, or straight to memory on a seam).
Each test prints its worst measured ratio of error to bound.
"""
import gc

import numpy as np
import pytest
import torch

import cubemap_cases as cc
import deferred_pipeline as dp
import lighting_cases
from dirt_amd import _lib, deferred, lighting

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fused_node(y, cls="_SampleCubemapFn"):
    """y comes from the fused autograd function `cls` (directly, or through the [0] of an unbatched call)"""
    assert y.grad_fn is not None
    names = [y.grad_fn.name()] + [fn.name() for fn, _ in y.grad_fn.next_functions if fn is not None]
    assert any(cls in n for n in names), names


def _run(inputs, needs=(True, True)):
    """-> (texels, valid, grad_cubemap or None, grad_directions or None) as numpy"""
    cubemap, d, mask, grad = inputs
    ct, dt = _gpu(cubemap).requires_grad_(needs[0]), _gpu(d).requires_grad_(needs[1])
    texels, valid = deferred.sample_cubemap(ct, dt, _gpu(mask))
    assert not valid.requires_grad
    if any(needs):
        _fused_node(texels)
        texels.backward(_gpu(grad))
    torch.cuda.synchronize()
    return (texels.detach().cpu().numpy(), valid.cpu().numpy(), None if ct.grad is None else ct.grad.cpu().numpy(),
            None if dt.grad is None else dt.grad.cpu().numpy())


def _ratio(err, bound, tag):
    """worst err / bound; where the bound is 0 the error must be"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    zero = bound == 0
    assert not np.any(err[zero]), tag
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _check_forward(got, fwd, tag):
    texels, valid = got[0], got[1]
    assert valid.dtype == np.bool_ and valid.shape == fwd["valid"].shape + (1,), tag
    assert np.array_equal(valid[..., 0], fwd["valid"]), tag
    assert np.array_equal(_bits(texels), _bits(fwd["texels"])), tag
    assert not np.any(_bits(texels)[~fwd["valid"]]), tag


def _check_grads(got, vjp, C, tag):
    """-> worst ratios (grad_cubemap, grad_directions) of error to bound, of the gradients present"""
    rc = rd = 0.0
    if got[2] is not None:
        assert got[2].shape == vjp["grad_cubemap"].shape, tag
        rc = _ratio(np.abs(got[2] - vjp["grad_cubemap"]), cc.cubemap_bound(vjp), tag)
        assert rc <= 1.0, (tag, "grad_cubemap", rc)
    if got[3] is not None:
        rd = _ratio(np.abs(got[3] - vjp["grad_directions"]), cc.directions_bound(vjp, C), tag)
        assert rd <= 1.0, (tag, "grad_directions", rd)
    return rc, rd


@pytest.mark.parametrize("ident", cc.CASE_IDS)
def test_matches_the_statement(ident):
    inputs, fwd, vjp = cc.case(ident)
    C = inputs[0].shape[-1]
    first, second = _run(inputs), _run(inputs)
    _check_forward(first, fwd, ident)
    assert np.array_equal(_bits(first[3]), _bits(second[3])), ident  # grad_directions: no run-to-run difference
    assert not np.any(_bits(first[3])[~fwd["valid"]]), ident
    rc, rd = _check_grads(first, vjp, C, ident)
    rc2, _ = _check_grads(second, vjp, C, ident)
    print("cubemap %s: grad_cubemap %.3f of its bound, grad_directions %.3f of its bound" % (ident, max(rc, rc2), rd))


@pytest.mark.parametrize("kind,C,frames", [(kind, C, frames) for C, frames in ((2, 1), (3, 2), (5, 1), (8, 2))
                                           for kind in ("patch", "direct")])
def test_exact_scatter(kind, C, frames):
    """Weights in {0, 1/4, 1/2, 1}, |ma| = 1 and small integer texels and cotangents: every partial sum is exact in
    float32, so both gradients equal the statement exactly whatever the order of the atomics -- through the LDS patch
    and its flush (patch), straight to memory on random faces (direct), and summed over the frames of the shared
    cube map (frames = 2)."""
    inputs, fwd, vjp = cc.exact_scatter_case(kind, C, frames)
    got = _run(inputs)
    _check_forward(got, fwd, kind)
    assert np.array_equal(got[2].astype(np.float64), vjp["grad_cubemap"]), kind
    assert np.array_equal(got[3].astype(np.float64), vjp["grad_directions"]), kind
    assert np.count_nonzero(vjp["grad_cubemap"]) > 0 and np.count_nonzero(vjp["grad_directions"]) > 0


@pytest.mark.parametrize("needs", [(False, False), (True, False), (False, True)], ids=["none", "cubemap", "directions"])
def test_gradient_subsets(needs):
    """Only the cube map, only the directions, neither: the requested gradient as the both-run's (grad_directions bit
    for bit, grad_cubemap within the bound), the others None."""
    ident = "17x33-s5-c3-perframe-random-bg"
    inputs, fwd, vjp = cc.case(ident)
    got, full = _run(inputs, needs), _run(inputs)
    _check_forward(got, fwd, ident)
    assert (got[2] is not None) == needs[0] and (got[3] is not None) == needs[1]
    _check_grads(got, vjp, 3, "subset %s" % (needs,))
    if needs[1]:
        assert np.array_equal(_bits(got[3]), _bits(full[3]))
    if needs[0]:
        assert np.all(np.abs(got[2] - full[2]) <= 2 * cc.cubemap_bound(vjp))


def test_forms(monkeypatch):
    """[H,W,3] with a shared cube map, non-contiguous views, bool and integer masks run the fused kernels; float64
    and DIRT_FUSED_DEFERRED=0 take the statement, with no fused node."""
    ident = "15x17-s5-c3-shared-lattice"
    (cubemap, d, _, grad), _, _ = cc.case(ident)
    mask = (np.random.default_rng(2).random(d.shape[:-1]) < 0.7).astype(np.uint8)
    fwd = cc.sample(cubemap, d, mask)
    vjp = cc.sample_vjp(cubemap, grad, fwd)
    base = _run((cubemap, d, mask, grad))
    _check_forward(base, fwd, ident)
    _check_grads(base, vjp, 3, ident)
    # unbatched, bool mask
    ct, dt = _gpu(cubemap).requires_grad_(True), _gpu(d[0]).requires_grad_(True)
    texels, valid = deferred.sample_cubemap(ct, dt, _gpu(mask[0]).bool())
    _fused_node(texels)
    assert texels.shape == (15, 17, 3) and valid.shape == (15, 17, 1) and valid.dtype == torch.bool
    texels.backward(_gpu(grad[0]))
    assert np.array_equal(_bits(texels.detach().cpu().numpy()), _bits(base[0][0]))
    assert np.array_equal(_bits(dt.grad.cpu().numpy()), _bits(base[3][0]))
    assert np.all(np.abs(ct.grad.cpu().numpy() - vjp["grad_cubemap"]) <= cc.cubemap_bound(vjp))
    # non-contiguous views, integer mask
    wide_c, wide_d = torch.zeros((6, 5, 5, 6), device=DEV), torch.zeros((1, 15, 17, 6), device=DEV)
    wide_c[..., ::2], wide_d[..., ::2] = _gpu(cubemap), _gpu(d)
    wide_c.requires_grad_(True), wide_d.requires_grad_(True)
    assert not wide_c[..., ::2].is_contiguous()
    texels, valid = deferred.sample_cubemap(wide_c[..., ::2], wide_d[..., ::2], _gpu(mask).long())
    _fused_node(texels)
    texels.backward(_gpu(grad))
    assert np.array_equal(_bits(texels.detach().cpu().numpy()), _bits(base[0]))
    assert np.array_equal(_bits(wide_d.grad.cpu().numpy()[..., ::2]), _bits(base[3]))
    assert float(wide_d.grad[..., 1::2].abs().max()) == 0.0 and float(wide_c.grad[..., 1::2].abs().max()) == 0.0
    assert np.all(np.abs(wide_c.grad.cpu().numpy()[..., ::2] - vjp["grad_cubemap"]) <= cc.cubemap_bound(vjp))
    # float64 and the switch: the framework-op statement
    f64 = cc.sample(cubemap, d, mask, np.float64)
    c64 = _gpu(cubemap).double().requires_grad_(True)
    y64, v64 = deferred.sample_cubemap(c64, _gpu(d).double(), _gpu(mask))
    assert "_SampleCubemapFn" not in y64.grad_fn.name()
    assert np.abs(y64.detach().cpu().numpy() - f64["texels"]).max() <= 1e-12
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    ct = _gpu(cubemap).requires_grad_(True)
    y, v = deferred.sample_cubemap(ct, _gpu(d), _gpu(mask))
    assert "_SampleCubemapFn" not in y.grad_fn.name()
    assert np.array_equal(v.cpu().numpy()[..., 0], fwd["valid"])
    # (four roundings on any path from a texel to the output, whatever the framework's kernels contract)
    assert np.abs(y.detach().cpu().numpy() - fwd["texels"]).max() <= 5 * 2.0 ** -24 * np.abs(cubemap).max()


def test_fused_backward_refuses_double_backward(monkeypatch):
    (cubemap, d, _, _), _, _ = cc.case("15x17-s5-c3-shared-lattice")
    ct, dt = _gpu(cubemap).requires_grad_(True), _gpu(d).requires_grad_(True)
    texels, _ = deferred.sample_cubemap(ct, dt)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(texels.square().sum(), [ct], create_graph=True)
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    texels, _ = deferred.sample_cubemap(ct, dt)
    g, = torch.autograd.grad(texels.square().sum(), [dt], create_graph=True)
    gg, = torch.autograd.grad(g.square().sum(), [ct])
    assert bool(torch.isfinite(gg).all())


def test_offsets_past_2_31():
    """One shared cube map [6, 8192, 8192, 6]: 2.42e9 elements, so the end of face 5 lies past a signed 32-bit offset
    while face 0 lies below it.  Four 4 x 4 frames probe half-texel directions (weights in {0, 1/4, 1/2, 1}, |ma| = 1,
    no tie of the major axis): the first corner of face 0 alone and the last corner of face 5 alone (their boxes fit
    the LDS patch, the second flushed past 2^31), and the four corners of face 0 and of face 5 (boxes as large as the
    face: straight to memory).  Forward and grad_cubemap on the corner blocks against the statement, exactly, and
    nothing else nonzero.  Two 9.7 GB tensors are alive at a time and the allocator's blocks are released at the
    end."""
    B, T, C = 4, 8192, 6
    assert 6 * T * T * C > 2 ** 31 > 5 * T * T * C  # (face 5 starts below the last int32 offset and ends past it)
    rng = np.random.default_rng(17)
    # x = k / 2 - 0.5: the taps lie on texels 0..1 and T-2..T-1; k = 0 and 2T would tie the major axis
    ks = np.array([1, 2, 2 * T - 3, 2 * T - 2, 2 * T - 1])
    pick = rng.integers(0, 5, (B, 4, 4, 2))
    pick[0] = rng.integers(0, 2, (4, 4, 2))      # the first frame: the first corner of face 0 alone
    pick[B - 1] = rng.integers(2, 5, (4, 4, 2))  # the last frame: the last corner of face 5 alone
    pick[B - 1, 3, 3] = 4                        # the last texel of the cube map
    pick[0, 0, 0] = 0                            # the first
    face = np.array([0, 0, 5, 5])[:, None, None]
    d = cc.on_face(face, ks[pick[..., 0]] / (2.0 * T), ks[pick[..., 1]] / (2.0 * T)).astype(np.float32)
    d[1, 1, 1] = -np.inf
    grad = rng.integers(1, 4, (B, 4, 4, C)).astype(np.float32)
    lib, stream = _lib.load(), torch.cuda.current_stream(DEV).cuda_stream
    corner = [slice(0, 2), slice(T - 2, T)]
    try:
        cubemap = torch.zeros((6, T, T, C), device=DEV)
        for k in (0, 5):
            for ys in corner:
                for xs in corner:
                    cubemap[k, ys, xs] = _gpu(rng.integers(1, 5, (2, 2, C)).astype(np.float32))

        def fetch(f, k, i, j):
            k, i, j = (torch.from_numpy(np.broadcast_to(a, i.shape).copy()).to(DEV) for a in (k, i, j))
            return cubemap[k, i, j].cpu().numpy()

        fwd = cc.sample((1, 6, T, T, C), d, None, fetch=fetch)
        assert np.array_equal(fwd["face"][fwd["valid"]], np.broadcast_to(face, (B, 4, 4))[fwd["valid"]])
        disp = cc.dispositions(fwd)
        assert disp["patch"] == 2 and disp["direct_box"] == 2
        dt_, gt_ = _gpu(d), _gpu(grad)
        texels = torch.empty((B, 4, 4, C), device=DEV)
        valid = torch.empty((B, 4, 4), dtype=torch.uint8, device=DEV)
        _lib.check(lib.dirt_texture_sample_cube_fwd(cubemap.data_ptr(), 1, T, C, dt_.data_ptr(), None, B, 4, 4,
                                                    texels.data_ptr(), valid.data_ptr(), stream))
        assert np.array_equal(valid.cpu().numpy() != 0, fwd["valid"]) and not fwd["valid"][1, 1, 1]
        assert np.array_equal(_bits(texels.cpu().numpy()), _bits(fwd["texels"]))
        assert int(np.count_nonzero(fwd["texels"])) == C * (B * 16 - 1)
        grad_cubemap = torch.empty_like(cubemap)  # (uninitialised: the call zero-fills it)
        grad_d = torch.empty((B, 4, 4, 3), device=DEV)
        _lib.check(lib.dirt_texture_sample_cube_bwd(cubemap.data_ptr(), 1, T, C, dt_.data_ptr(), None, B, 4, 4,
                                                    gt_.data_ptr(), grad_cubemap.data_ptr(), grad_d.data_ptr(),
                                                    stream))
        torch.cuda.synchronize()
        # the statement's scatter on the corner blocks alone (every tap lies in one)
        want = np.zeros((6, 4, 4, C))
        fold = lambda i: np.where(i < 2, i, i - (T - 4))  # noqa: E731  (0, 1, T-2, T-1 -> 0, 1, 2, 3)
        v = fwd["valid"]
        for ii, jj, w in ((fwd["i0"], fwd["j0"], fwd["oma"] * fwd["omb"]), (fwd["i0"], fwd["j1"], fwd["a"] * fwd["omb"]),
                          (fwd["i1"], fwd["j0"], fwd["oma"] * fwd["b"]), (fwd["i1"], fwd["j1"], fwd["a"] * fwd["b"])):
            assert np.all((ii[v] < 2) | (ii[v] >= T - 2)) and np.all((jj[v] < 2) | (jj[v] >= T - 2))
            np.add.at(want, (fwd["face"][v], fold(ii[v]), fold(jj[v])),
                      grad[v].astype(np.float64) * w[v][:, None].astype(np.float64))
        for k in range(6):
            got = torch.cat([torch.cat([grad_cubemap[k, ys, xs] for xs in corner], 1) for ys in corner], 0)
            assert np.array_equal(got.cpu().numpy().astype(np.float64), want[k]), k
            assert int(torch.count_nonzero(grad_cubemap[k])) == int(np.count_nonzero(want[k])), k
        assert np.count_nonzero(want[5, 3, 3]) == C and np.count_nonzero(want[0, 0, 0]) == C
        assert not np.any(want[1:5])
        assert bool(torch.isfinite(grad_d).all()) and not bool(grad_d[1, 1, 1].any())
    finally:
        cubemap = grad_cubemap = None
        gc.collect()
        torch.cuda.empty_cache()


def test_captures_into_a_graph():
    """One forward and backward captured with torch.cuda.graph on one stream (no parallel branches; the zero-fill of
    grad_cubemap is an asynchronous memset on it), replayed after the directions and the cube map changed in place:
    equal to the eager result, grad_directions bit for bit, grad_cubemap within the bound."""
    first = cc.case("17x33-s64-c3-shared-oneface-magnify-bg")[0]
    other = cc.case("17x33-s64-c3-shared-corner-bg")[0]
    second = (np.random.default_rng(21).standard_normal(first[0].shape).astype(np.float32), other[1], None, other[3])
    fwd2 = cc.sample(*second[:3])
    vjp2 = cc.sample_vjp(second[0], second[3], fwd2)
    assert 0.2 < fwd2["valid"].mean() < 0.9 and np.count_nonzero(vjp2["grad_cubemap"]) > 100
    ct, dt = _gpu(first[0]).requires_grad_(True), _gpu(first[1]).requires_grad_(True)
    g = _gpu(second[3])
    out = {}

    def step():
        texels, valid = deferred.sample_cubemap(ct, dt)
        out["texels"], out["valid"] = texels, valid
        out["grads"] = torch.autograd.grad(texels, [ct, dt], g)

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
        ct.copy_(_gpu(second[0]))
        dt.copy_(_gpu(second[1]))
    graph.replay()
    torch.cuda.synchronize()
    got = (out["texels"].detach().cpu().numpy(), out["valid"].cpu().numpy(), out["grads"][0].cpu().numpy(),
           out["grads"][1].cpu().numpy())
    del graph
    out.clear()
    eager = _run(second)
    _check_forward(got, fwd2, "graph")
    assert np.array_equal(_bits(got[0]), _bits(eager[0])) and np.array_equal(got[1], eager[1])
    assert np.array_equal(_bits(got[3]), _bits(eager[3]))
    rc, rd = _check_grads(got, vjp2, 3, "graph")
    print("graph replay: grad_cubemap %.3f of its bound, grad_directions %.3f of its bound" % (rc, rd))


def test_chain_environment_mapped_shading():
    """The deferred chain at 64 x 64 over dp.grid_surface(n=12) with an environment: the position and normal
    G-buffers dilated, zero-filled where they stay background, the unit view ray i to the position and the reflection
    vector r = i - 2 (n . i) n formed with framework ops, r looked up in an 8 x 8 x 3 cube map under the mask of the
    covered pixels, and the texels added to deferred.shade's pixels.  The fused lookup against `_sample_cubemap_ops`
    on the GPU, everything else shared (the vertex normals computed once: their sum uses float atomics): valid equal;
    texels bit-equal to the numpy statement at the fused path's own directions; d loss / d cubemap within the scatter
    bound of the statement and within 1e-4 of its scale from the framework ops' (tests/lighting_cases.py's
    GRAD_FRAC); d loss / d world vertices within 1e-2 in relative L2 (the tolerance of the textured chain test).
    Measured on an MI355X: the lookups fall on four faces; d loss / d cubemap 0.214 of the scatter bound and 4.8e-7 of
    its scale from the framework ops', d loss / d world vertices 1.1e-7 in relative L2."""
    H = W = 64
    world, faces, albedo = dp.grid_surface(n=12)
    f, al = _gpu(faces), _gpu(albedo)
    wts = torch.rand((H, W, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    env0 = torch.rand((6, 8, 8, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 0.8 + 0.2
    grey, ld, red, white = dp._constants(DEV)
    cam = dp.camera_position(H, W, DEV)
    normals = lighting.vertex_normals(_gpu(world), f).detach()

    def chain(lookup):
        Vw, env = _gpu(world).requires_grad_(True), env0.clone().requires_grad_(True)
        pos, col, nrm, _ = dp.gbuffers(dp.hip_render, Vw, f, al, H, W, normals=normals)
        bg = torch.isinf(pos).any(-1)
        pos_d, nrm_d = deferred.dilate(pos, bg), deferred.dilate(nrm, bg)
        covered = torch.isfinite(pos_d).all(-1, keepdim=True) & torch.isfinite(nrm_d).all(-1, keepdim=True)
        pos_s, nrm_s = torch.where(covered, pos_d, 0.0), torch.where(covered, nrm_d, 0.0)
        ray = pos_s - cam
        i = ray / torch.linalg.norm(ray, dim=-1, keepdim=True)
        r = i - 2.0 * (nrm_s * i).sum(-1, keepdim=True) * nrm_s
        texels, sampled = lookup(env, r, covered[..., 0])
        shaded, valid = deferred.shade(pos, col, nrm, grey, ld, red, white, cam, 6., False)
        pixels = shaded + texels
        loss = dp.loss_fn(pixels, valid, wts)
        g_env, g_v = torch.autograd.grad(loss, [env, Vw], retain_graph=True)
        g_tex, = torch.autograd.grad(loss, [texels])
        return dict(valid=valid, sampled=sampled, texels=texels, r=r.detach(), covered=covered[..., 0], g_env=g_env,
                    g_v=g_v, g_tex=g_tex)

    fused = chain(lambda e, r, m: deferred.sample_cubemap(e, r, m))
    _fused_node(fused["texels"])
    ops = chain(lambda e, r, m: deferred._sample_cubemap_ops(e, r, m))
    assert torch.equal(fused["valid"], ops["valid"]) and torch.equal(fused["sampled"], ops["sampled"])
    assert torch.equal(fused["r"], ops["r"])
    assert bool(fused["sampled"].any()) and not bool(fused["sampled"].all())
    assert torch.equal(fused["sampled"], fused["valid"])
    # the statement at the fused path's own directions
    fwd = cc.sample(env0.cpu().numpy(), fused["r"].cpu().numpy()[None], fused["covered"].cpu().numpy()[None])
    assert np.array_equal(fwd["valid"][0], fused["sampled"].cpu().numpy()[..., 0])
    assert len(set(fwd["face"][fwd["valid"]].tolist())) >= 2
    assert np.array_equal(_bits(fused["texels"].detach().cpu().numpy()), _bits(fwd["texels"][0]))
    vjp = cc.sample_vjp(env0.cpu().numpy(), fused["g_tex"].cpu().numpy()[None], fwd)
    r_env = _ratio(np.abs(fused["g_env"].cpu().numpy() - vjp["grad_cubemap"]), cc.cubemap_bound(vjp), "chain cubemap")
    scale = float(ops["g_env"].abs().max())
    d_env = float((fused["g_env"] - ops["g_env"]).abs().max()) / scale
    rel_l2 = float(torch.linalg.norm(fused["g_v"] - ops["g_v"]) / torch.linalg.norm(ops["g_v"]))
    print("environment chain 64x64: d loss / d cubemap %.3f of the scatter bound (%.3g of its scale from the framework "
          "ops'), d loss / d world vertices rel L2 %.3g, faces %s"
          % (r_env, d_env, rel_l2, sorted(set(fwd["face"][fwd["valid"]].tolist()))))
    assert r_env <= 1.0
    assert scale > 0 and d_env <= lighting_cases.GRAD_FRAC
    assert bool(torch.isfinite(fused["g_v"]).all()) and float(ops["g_v"].abs().max()) > 0
    assert rel_l2 < 1e-2, rel_l2
