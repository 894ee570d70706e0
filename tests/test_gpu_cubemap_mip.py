"""The fused seamless mip-mapped cube-map kernels (dirt_amd/csrc/cubemap_mip_kernels.h through
dirt_amd.deferred.build_cubemap_mipmaps / sample_cubemap_mip) against the numpy statement of record
(tests/cubemap_mip_cases.py) on its whole table.

Forward, valid and the stored lod: bit-exact against the float32 statement, unsampled pixels exactly 0.
grad_directions and grad_lod: bit-identical between two runs (gathers in a fixed order), zero at unsampled pixels, and
within k * 2^-24 * (sum of the absolute terms) of the float64 statement, k = C + 13 and C + 9
(cubemap_mip_cases.directions_roundings, lod_roundings).
grad_packed: within (n + 4) * 2^-24 * S per element (the texture scatter's bound with the level weight's and the
corner third's roundings), whichever way a tile is summed; grad_cubemap: that bound carried through the chain's
backward.
Each test prints its worst measured ratio of error to bound.
"""
import gc

import numpy as np
import pytest
import torch

import cubemap_cases as cc
import cubemap_mip_cases as cm
import deferred_pipeline as dp
import lighting_cases
from dirt_amd import _lib, deferred, lighting

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FN = "_SampleCubemapMipFn"


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fused_node(y, cls=FN):
    """y comes from the fused autograd function `cls` (directly, or through the [0] of an unbatched call)"""
    assert y.grad_fn is not None
    names = [y.grad_fn.name()] + [fn.name() for fn, _ in y.grad_fn.next_functions if fn is not None]
    assert any(cls in n for n in names), names


def _run(inp, needs=(True, True, True)):
    """needs = (the cube map, through the chain; the directions; an explicit lod) -> dict of numpy arrays: texels,
    valid, lod, and grad_packed, grad_cubemap, grad_directions, grad_lod (None where not asked for)"""
    ct = _gpu(inp["cubemap"]).requires_grad_(needs[0])
    dt = _gpu(inp["directions"]).requires_grad_(needs[1])
    lt = None if inp["lod"] is None else _gpu(inp["lod"]).requires_grad_(needs[2])
    chain = deferred.build_cubemap_mipmaps(ct)
    if needs[0]:
        assert "_BuildMipmapsFn" in "".join([chain.packed.grad_fn.name()] + [
            fn.name() for fn, _ in chain.packed.grad_fn.next_functions if fn is not None])
        chain.packed.retain_grad()
    texels, valid, lod = deferred._sample_cubemap_mip(chain, dt, _gpu(inp["mask"]), lt, inp["lod_bias"],
                                                      inp["seamless"])
    assert not valid.requires_grad and not lod.requires_grad
    if any(needs[:2]) or (needs[2] and lt is not None):
        _fused_node(texels)
        texels.backward(_gpu(inp["grad"]))
    torch.cuda.synchronize()
    out = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    return dict(texels=out(texels), valid=valid.cpu().numpy(), lod=out(lod), grad_packed=out(chain.packed.grad),
                grad_cubemap=out(ct.grad), grad_directions=out(dt.grad), grad_lod=None if lt is None else out(lt.grad))


def _ratio(err, bound, tag):
    """worst err / bound; where the bound is 0 the error must be"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    zero = bound == 0
    assert not np.any(err[zero]), tag
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _check_forward(got, fwd, tag):
    assert got["valid"].dtype == np.bool_ and got["valid"].shape == fwd["valid"].shape + (1,), tag
    assert np.array_equal(got["valid"][..., 0], fwd["valid"]), tag
    assert np.array_equal(_bits(got["lod"]), _bits(fwd["lod"])), tag
    assert np.array_equal(_bits(got["texels"]), _bits(fwd["texels"])), tag
    assert not np.any(_bits(got["texels"])[~fwd["valid"]]), tag


def _check_grads(got, vjp, C, tag):
    """-> worst ratios (grad_packed, grad_cubemap, grad_directions, grad_lod) of error to bound, of those present"""
    r = [0.0, 0.0, 0.0, 0.0]
    for n, (key, bound) in enumerate((("grad_packed", cm.packed_bound(vjp)), ("grad_cubemap", vjp["cubemap_bound"]),
                                      ("grad_directions", cm.directions_bound(vjp, C)),
                                      ("grad_lod", cm.lod_bound(vjp, C)))):
        if got[key] is not None:
            assert got[key].shape == vjp[key].shape, (tag, key)
            r[n] = _ratio(np.abs(got[key] - vjp[key]), bound, (tag, key))
            assert r[n] <= 1.0, (tag, key, r[n])
    return r


def _same_gathers(a, b, fwd, tag):
    for key in ("grad_directions", "grad_lod"):
        if a[key] is not None:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (tag, key)  # no run-to-run difference
            assert not np.any(_bits(a[key])[~fwd["valid"]]), (tag, key)


@pytest.mark.parametrize("ident", cm.CASE_IDS)
def test_matches_the_statement(ident):
    """Measured on an MI355X over the 84 cases (one run): grad_packed at most 0.481 of its bound, grad_cubemap 0.279,
    grad_directions 0.259, grad_lod 0.176; the forward, valid and the lod bit-exact, the gathers bit-identical between
    the two runs of every case."""
    inp, _, fwd, vjp = cm.case(ident)
    C = inp["cubemap"].shape[-1]
    first, second = _run(inp), _run(inp)
    _check_forward(first, fwd, ident)
    _same_gathers(first, second, fwd, ident)
    r1, r2 = _check_grads(first, vjp, C, ident), _check_grads(second, vjp, C, ident)
    print("cubemap mip %s: grad_packed %.3f, grad_cubemap %.3f, grad_directions %.3f, grad_lod %.3f of their bounds"
          % (ident, max(r1[0], r2[0]), max(r1[1], r2[1]), r1[2], r1[3]))


@pytest.mark.parametrize("kind,C,frames", [(kind, C, frames) for C, frames in ((2, 1), (3, 2), (5, 1), (8, 2))
                                           for kind in ("box", "memory", "whole")])
def test_exact_scatter(kind, C, frames):
    """Half-texel directions with |ma| = 1, lods in {integer, integer + 1/2}, small integer texels and cotangents,
    no corner tap: every partial sum is exact in float32, so the three gradients (and the cube map's through the
    chain) equal the statement exactly whatever the order of the atomics -- through one face's boxes in LDS (box),
    straight to memory with folded taps (memory), through a whole level in LDS (whole), and summed over the frames of
    the shared chain (frames = 2)."""
    inp, _, fwd, vjp = cm.exact_scatter_case(kind, C, frames)
    got = _run(inp)
    _check_forward(got, fwd, kind)
    for key in ("grad_packed", "grad_cubemap", "grad_directions", "grad_lod"):
        assert np.array_equal(got[key].astype(np.float64), vjp[key]), (kind, key)
        assert np.count_nonzero(vjp[key]) > 0, (kind, key)


@pytest.mark.parametrize("S,C", [(1, 3), (2, 8), (1, 6)])
def test_corner_pixels(S, C):
    """Two 16 x 16 frames over a shared S x S cube map at every level of its chain: with S = 1 every pixel has a corner
    tap, with S = 2 those of its 1 x 1 level and of the corner cells of its 2 x 2 level.  The corner third is no
    dyadic number, so these are held to the bounds, not to equality.  Measured on an MI355X (grad_packed, grad_cubemap,
    grad_directions, grad_lod): S = 1, C = 3: 0.001, 0.001, 0.161, 0 (one level: no lod gradient); S = 2, C = 8: 0.024,
    0.007, 0.108, 0.081; S = 1, C = 6: 0.002, 0.002, 0.098, 0."""
    rng = np.random.default_rng(31 + S + C)
    shape = (2, 16, 16)
    L = len(cm.build_chain(np.zeros((6, S, S, 1), np.float32)))
    inp = dict(cubemap=rng.standard_normal((6, S, S, C)).astype(np.float32),
               directions=rng.standard_normal(shape + (3,)).astype(np.float32), mask=None,
               lod=rng.uniform(-0.2, L - 0.8, shape).astype(np.float32), lod_bias=0.0, seamless=True,
               grad=rng.standard_normal(shape + (C,)).astype(np.float32))
    chain, fwd, vjp = cm.statement(inp)
    corners = sum(int(((np.asarray(lv["kind"]) == 2).any(0) & lv["sel"]).sum()) for lv in fwd["levels"].values())
    assert corners >= (512 if S == 1 else 100)
    first, second = _run(inp), _run(inp)
    _check_forward(first, fwd, S)
    _same_gathers(first, second, fwd, S)
    r = _check_grads(first, vjp, C, S)
    print("corner pixels S = %d, C = %d (%d corner taps): grad_packed %.3f, grad_cubemap %.3f, grad_directions %.3f, "
          "grad_lod %.3f of their bounds" % ((S, C, corners) + tuple(r)))


SUBSETS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]


@pytest.mark.parametrize("needs", SUBSETS, ids=["".join(n for n, on in zip("cdl", needs) if on) or "none"
                                                for needs in SUBSETS])
def test_gradient_subsets(needs):
    """Every subset of {chain, directions, lod}: the requested gradients as the run of all three (the gathers bit for
    bit, the scatter within the bound), the others None."""
    ident = "17x33-s64-c3-shared-corner-frac-bg"
    inp, _, fwd, vjp = cm.case(ident)
    got, full = _run(inp, needs), _run(inp)
    _check_forward(got, fwd, ident)
    assert (got["grad_cubemap"] is not None) == needs[0] and (got["grad_packed"] is not None) == needs[0]
    assert (got["grad_directions"] is not None) == needs[1] and (got["grad_lod"] is not None) == needs[2]
    _check_grads(got, vjp, 3, "subset %s" % (needs,))
    for key in ("grad_directions", "grad_lod"):
        if got[key] is not None:
            assert np.array_equal(_bits(got[key]), _bits(full[key])), key
    if needs[0]:
        assert np.all(np.abs(got["grad_packed"] - full["grad_packed"]) <= 2 * cm.packed_bound(vjp))


def test_forms(monkeypatch):
    """[H,W,3] with a shared chain, non-contiguous views, bool and integer masks and a float64 lod tensor run the
    fused kernels; float64 operands and DIRT_FUSED_DEFERRED=0 take the statement, with no fused node."""
    ident = "15x17-s8-c3-shared-lattice-frac"
    inp = dict(cm.case_input(ident))
    inp["mask"] = (np.random.default_rng(2).random(inp["directions"].shape[:-1]) < 0.7).astype(np.uint8)
    chain, fwd, vjp = cm.statement(inp)
    base = _run(inp)
    _check_forward(base, fwd, ident)
    _check_grads(base, vjp, 3, ident)
    cubemap, d, mask, lod, grad = (inp[k] for k in ("cubemap", "directions", "mask", "lod", "grad"))
    # unbatched, bool mask, a float64 lod: its gradient comes back in float64
    ct, dt = _gpu(cubemap).requires_grad_(True), _gpu(d[0]).requires_grad_(True)
    lt = _gpu(lod[0]).double().requires_grad_(True)
    texels, valid = deferred.sample_cubemap_mip(ct, dt, _gpu(mask[0]).bool(), lt)
    _fused_node(texels)
    assert texels.shape == (15, 17, 3) and valid.shape == (15, 17, 1) and valid.dtype == torch.bool
    texels.backward(_gpu(grad[0]))
    assert np.array_equal(_bits(texels.detach().cpu().numpy()), _bits(base["texels"][0]))
    assert np.array_equal(_bits(dt.grad.cpu().numpy()), _bits(base["grad_directions"][0]))
    assert lt.grad.dtype == torch.float64
    assert np.array_equal(_bits(lt.grad.float().cpu().numpy()), _bits(base["grad_lod"][0]))
    assert np.all(np.abs(ct.grad.cpu().numpy() - vjp["grad_cubemap"]) <= vjp["cubemap_bound"])
    # non-contiguous views, integer mask, a wrapped chain
    packed = _gpu(cm.pack(chain))
    wide_p = torch.zeros(packed.shape[:-1] + (6,), device=DEV)
    wide_d = torch.zeros((1, 15, 17, 6), device=DEV)
    wide_p[..., ::2], wide_d[..., ::2] = packed, _gpu(d)
    wide_p.requires_grad_(True), wide_d.requires_grad_(True)
    assert not wide_p[..., ::2].is_contiguous()
    wrapped = deferred.CubeMipmaps(wide_p[..., ::2], 8)
    texels, valid = deferred.sample_cubemap_mip(wrapped, wide_d[..., ::2], _gpu(mask).long(), _gpu(lod))
    _fused_node(texels)
    texels.backward(_gpu(grad))
    assert np.array_equal(_bits(texels.detach().cpu().numpy()), _bits(base["texels"]))
    assert np.array_equal(_bits(wide_d.grad.cpu().numpy()[..., ::2]), _bits(base["grad_directions"]))
    assert float(wide_d.grad[..., 1::2].abs().max()) == 0.0 and float(wide_p.grad[..., 1::2].abs().max()) == 0.0
    assert np.all(np.abs(wide_p.grad.cpu().numpy()[..., ::2] - vjp["grad_packed"]) <= cm.packed_bound(vjp))
    # float64 operands and the switch: the framework-op statement
    _, f64, _ = cm.statement(inp, np.float64)
    c64 = _gpu(cubemap).double().requires_grad_(True)
    y64, v64 = deferred.sample_cubemap_mip(c64, _gpu(d).double(), _gpu(mask), _gpu(lod).double())
    assert FN not in y64.grad_fn.name()
    assert np.abs(y64.detach().cpu().numpy() - f64["texels"]).max() <= 1e-12
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    ct = _gpu(cubemap).requires_grad_(True)
    y, v = deferred.sample_cubemap_mip(ct, _gpu(d), _gpu(mask), _gpu(lod))
    assert FN not in y.grad_fn.name()
    assert np.array_equal(v.cpu().numpy()[..., 0], fwd["valid"])
    # (a dozen roundings on any path from a texel to the output, whatever the framework's kernels contract)
    assert np.abs(y.detach().cpu().numpy() - fwd["texels"]).max() <= 16 * 2.0 ** -24 * np.abs(cubemap).max()


def test_fused_backward_refuses_double_backward(monkeypatch):
    inp = cm.case_input("15x17-s8-c3-shared-lattice-frac")
    ct, dt = _gpu(inp["cubemap"]).requires_grad_(True), _gpu(inp["directions"]).requires_grad_(True)
    lt = _gpu(np.nan_to_num(inp["lod"], nan=0.5, posinf=1.0)).requires_grad_(True)
    texels, _ = deferred.sample_cubemap_mip(ct, dt, None, lt)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(texels.square().sum(), [lt], create_graph=True)
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    texels, _ = deferred.sample_cubemap_mip(ct, dt, None, lt)
    g, gl = torch.autograd.grad(texels.square().sum(), [dt, lt], create_graph=True)
    gg, = torch.autograd.grad(g.square().sum() + gl.square().sum(), [ct])
    assert bool(torch.isfinite(gg).all())


def test_offsets_past_2_31():
    """One shared chain of 8192 x 8192 faces with 6 channels, wrapped zero-filled (no build): 6 * N * 6 = 3.22e9
    floats, so face 5's chain lies past a signed 32-bit offset and face 0's below it.  Four 4 x 4 frames at half-texel
    directions (|ma| = 1, every weight 1/4, or 1 at a face's centre): the first 2 x 2 texels of face 0 at lod 0 (one
    face's box in LDS, the first texel of the chain); the last 2 x 2 texels of face 5 at lod 0 (a box flushed past
    2^31); the centre of face 5 at lod 13, its 1 x 1 level (a whole level in LDS, the last texel of the chain, the
    folded and corner taps at weight 0); the corner blocks of faces 0 and 5 mixed (straight to memory).  Forward and
    grad_packed against hand-formed means and quarter sums, exactly, and nothing else nonzero.  Two 12.9 GB tensors
    are alive at a time and the allocator's blocks are released at the end."""
    B, T, C = 4, 8192, 6
    dims, offsets, N = cm.tmc.layout(T, T)
    L = len(dims)
    assert L == 14 and 6 * N * C > 2 ** 31 > N * C and 5 * N * C > 2 ** 31
    rng = np.random.default_rng(17)
    lo, hi = 2, 2 * T - 2   # x = k / 2 - 0.5: taps on texels 0..1 and T-2..T-1, each weight 1/2
    ku, kv = np.full((B, 4, 4), lo), np.full((B, 4, 4), lo)
    face = np.zeros((B, 4, 4), np.int64)
    ku[1] = kv[1] = hi
    face[1] = face[2] = 5
    ku[2] = kv[2] = T       # the centre of the face
    ku[3], kv[3] = rng.choice([lo, hi], (4, 4)), rng.choice([lo, hi], (4, 4))
    face[3] = rng.choice([0, 5], (4, 4))
    face[3, 0, 0], face[3, 0, 1] = 0, 5
    d = cc.on_face(face, ku / (2.0 * T), kv / (2.0 * T)).astype(np.float32)
    d[1, 1, 1] = -np.inf
    lod = np.zeros((B, 4, 4), np.float32)
    lod[2] = L - 1
    grad = rng.integers(1, 4, (B, 4, 4, C)).astype(np.float32)
    lib, stream = _lib.load(), torch.cuda.current_stream(DEV).cuda_stream
    block = {lo: slice(0, 2), hi: slice(T - 2, T)}
    try:
        packed = torch.zeros((6, N, C), device=DEV)
        chain = deferred.CubeMipmaps(packed, T)
        assert len(chain) == L and chain.level(0).shape == (6, T, T, C) and chain.level(L - 1).shape == (6, 1, 1, C)
        values = {}
        for f in (0, 5):
            for ky in (lo, hi):
                for kx in (lo, hi):
                    values[f, ky, kx] = rng.integers(1, 5, (2, 2, C)).astype(np.float32)
                    chain.level(0)[f, block[ky], block[kx]] = _gpu(values[f, ky, kx])
        top = rng.integers(1, 5, (C,)).astype(np.float32)
        chain.level(L - 1)[5, 0, 0] = _gpu(top)
        assert float(packed[5, N - 1, 0]) == top[0] and float(packed[0, 0, 0]) == values[0, lo, lo][0, 0, 0]
        want = np.zeros((B, 4, 4, C), np.float32)
        want_grad = {key: np.zeros((2, 2, C)) for key in values}
        want_top = np.zeros(C)
        for b in range(B):
            for y in range(4):
                for x in range(4):
                    if (b, y, x) == (1, 1, 1):
                        continue
                    if b == 2:
                        want[b, y, x] = top
                        want_top += grad[b, y, x]
                    else:
                        key = (int(face[b, y, x]), int(kv[b, y, x]), int(ku[b, y, x]))
                        want[b, y, x] = values[key].sum((0, 1)) * 0.25
                        want_grad[key] += grad[b, y, x] * 0.25
        dt_, gt_, lt_ = _gpu(d), _gpu(grad), _gpu(lod)
        texels = torch.empty((B, 4, 4, C), device=DEV)
        valid = torch.empty((B, 4, 4), dtype=torch.uint8, device=DEV)
        lod_out = torch.empty((B, 4, 4), device=DEV)
        _lib.check(lib.dirt_texture_sample_cube_mip_fwd(packed.data_ptr(), 1, T, C, 0, dt_.data_ptr(), None,
                                                        lt_.data_ptr(), 0.0, B, 4, 4, 1, texels.data_ptr(),
                                                        valid.data_ptr(), lod_out.data_ptr(), stream))
        ok = valid.cpu().numpy() != 0
        assert ok.sum() == B * 16 - 1 and not ok[1, 1, 1]
        assert np.array_equal(lod_out.cpu().numpy(), np.where(ok, lod, 0))
        assert np.array_equal(_bits(texels.cpu().numpy()), _bits(want))
        grad_packed = torch.empty_like(packed)  # (uninitialised: the call zero-fills it)
        grad_d = torch.empty((B, 4, 4, 3), device=DEV)
        grad_l = torch.empty((B, 4, 4), device=DEV)
        _lib.check(lib.dirt_texture_sample_cube_mip_bwd(packed.data_ptr(), 1, T, C, 0, dt_.data_ptr(), None,
                                                        lt_.data_ptr(), 0.0, lod_out.data_ptr(), B, 4, 4, 1,
                                                        gt_.data_ptr(), grad_packed.data_ptr(), grad_d.data_ptr(),
                                                        grad_l.data_ptr(), stream))
        torch.cuda.synchronize()
        got = deferred.CubeMipmaps(grad_packed, T)
        nonzero = 0
        for (f, ky, kx), w in want_grad.items():
            have = got.level(0)[f, block[ky], block[kx]].cpu().numpy().astype(np.float64)
            assert np.array_equal(have, w), (f, ky, kx)
            nonzero += int(np.count_nonzero(w))
        assert np.array_equal(got.level(L - 1)[5, 0, 0].cpu().numpy().astype(np.float64), want_top)
        assert float(grad_packed[5, N - 1, C - 1]) == want_top[C - 1] > 0
        assert float(grad_packed[0, 0, 0]) == want_grad[0, lo, lo][0, 0, 0] > 0
        assert int(torch.count_nonzero(grad_packed)) == nonzero + C
        assert bool(torch.isfinite(grad_d).all()) and not bool(grad_d[1, 1, 1].any())
        assert bool(torch.isfinite(grad_l).all()) and not bool(grad_l[2].any()) and not bool(grad_l[1, 1, 1].any())
    finally:
        packed = grad_packed = chain = got = None
        gc.collect()
        torch.cuda.empty_cache()


def test_captures_into_a_graph():
    """One chain build, lookup and backward captured with torch.cuda.graph on one stream (no parallel branches; the
    zero-fill of grad_packed is an asynchronous memset on it), replayed after the cube map, the directions and the lod
    changed in place: equal to the eager result, the gathers bit for bit, the scatter within the bound.  Measured on an
    MI355X: grad_packed 0.353, grad_cubemap 0.165, grad_directions 0.179, grad_lod 0.082 of their bounds."""
    first = cm.case_input("17x33-s64-c3-shared-oneface-magnify-frac-bg-bias-4.50")
    second = dict(cm.case_input("17x33-s64-c3-shared-corner-frac-bg"))
    second["lod_bias"] = first["lod_bias"]
    _, fwd2, vjp2 = cm.statement(second)
    assert 0.2 < fwd2["valid"].mean() < 0.9 and np.count_nonzero(vjp2["grad_packed"]) > 100
    ct, dt = _gpu(first["cubemap"]).requires_grad_(True), _gpu(first["directions"]).requires_grad_(True)
    lt = _gpu(first["lod"]).requires_grad_(True)
    g = _gpu(second["grad"])
    out = {}

    def step():
        chain = deferred.build_cubemap_mipmaps(ct)
        texels, valid, lod = deferred._sample_cubemap_mip(chain, dt, None, lt, first["lod_bias"], True)
        out["texels"], out["valid"], out["lod"] = texels, valid, lod
        out["grads"] = torch.autograd.grad(texels, [chain.packed, dt, lt], g, retain_graph=True)
        out["grad_cubemap"], = torch.autograd.grad(chain.packed, [ct], out["grads"][0])

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
        ct.copy_(_gpu(second["cubemap"]))
        dt.copy_(_gpu(second["directions"]))
        lt.copy_(_gpu(second["lod"]))
    graph.replay()
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    got = dict(texels=cpu(out["texels"]), valid=cpu(out["valid"]), lod=cpu(out["lod"]),
               grad_packed=cpu(out["grads"][0]), grad_cubemap=cpu(out["grad_cubemap"]),
               grad_directions=cpu(out["grads"][1]), grad_lod=cpu(out["grads"][2]))
    del graph
    out.clear()
    eager = _run(second)
    _check_forward(got, fwd2, "graph")
    assert np.array_equal(_bits(got["texels"]), _bits(eager["texels"]))
    _same_gathers(got, eager, fwd2, "graph")
    r = _check_grads(got, vjp2, 3, "graph")
    print("graph replay: grad_packed %.3f, grad_cubemap %.3f, grad_directions %.3f, grad_lod %.3f of their bounds"
          % tuple(r))


def test_chain_glossy_environment_mapped_shading():
    """test_gpu_cubemap's environment chain at 64 x 64 over dp.grid_surface(n=12) with a roughness G-buffer: the
    reflection vector looked up in the mip chain of an 8 x 8 x 3 cube map at lod = roughness * (levels - 1), the
    roughness a leaf that wants a gradient (0 over a quarter of the frame: an integer lod), and the texels added to
    deferred.shade's pixels.  The fused lookup against `_sample_cubemap_mip_ops` on the GPU, everything else shared:
    valid equal; texels bit-equal to the numpy statement at the fused path's own directions; d loss / d cubemap
    within the statement's bound and within lighting_cases.GRAD_FRAC of its scale from the framework ops'; d loss / d
    roughness within its bound and within GRAD_FRAC of its scale; d loss / d world vertices within 1e-2 in relative
    L2.  Measured on an MI355X: d loss / d cubemap 0.047 of its bound and 1.7e-7 of its scale from the framework ops',
    d loss / d roughness 0.117 of its bound and 1.3e-7 of its scale, d loss / d world vertices 7.3e-8 in relative L2."""
    H = W = 64
    world, faces, albedo = dp.grid_surface(n=12)
    f, al = _gpu(faces), _gpu(albedo)
    wts = torch.rand((H, W, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    env0 = torch.rand((6, 8, 8, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 0.8 + 0.2
    rough0 = torch.rand((H, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    rough0[: H // 2, : W // 2] = 0.0
    grey, ld, red, white = dp._constants(DEV)
    cam = dp.camera_position(H, W, DEV)
    normals = lighting.vertex_normals(_gpu(world), f).detach()

    def chain(lookup):
        Vw, env = _gpu(world).requires_grad_(True), env0.clone().requires_grad_(True)
        rough = rough0.clone().requires_grad_(True)
        pos, col, nrm, _ = dp.gbuffers(dp.hip_render, Vw, f, al, H, W, normals=normals)
        bg = torch.isinf(pos).any(-1)
        pos_d, nrm_d = deferred.dilate(pos, bg), deferred.dilate(nrm, bg)
        covered = torch.isfinite(pos_d).all(-1, keepdim=True) & torch.isfinite(nrm_d).all(-1, keepdim=True)
        pos_s, nrm_s = torch.where(covered, pos_d, 0.0), torch.where(covered, nrm_d, 0.0)
        ray = pos_s - cam
        i = ray / torch.linalg.norm(ray, dim=-1, keepdim=True)
        r = i - 2.0 * (nrm_s * i).sum(-1, keepdim=True) * nrm_s
        mips = deferred.build_cubemap_mipmaps(env)
        lod = rough * float(len(mips) - 1)
        texels, sampled = lookup(mips, r, covered[..., 0], lod)[:2]
        shaded, valid = deferred.shade(pos, col, nrm, grey, ld, red, white, cam, 6., False)
        pixels = shaded + texels
        loss = dp.loss_fn(pixels, valid, wts)
        g_env, g_v, g_rough = torch.autograd.grad(loss, [env, Vw, rough], retain_graph=True)
        g_tex, = torch.autograd.grad(loss, [texels])
        return dict(valid=valid, sampled=sampled, texels=texels, r=r.detach(), covered=covered[..., 0], g_env=g_env,
                    g_v=g_v, g_rough=g_rough, g_tex=g_tex, lod=lod.detach())

    fused = chain(lambda m, r, c, l: deferred.sample_cubemap_mip(m, r, c, l))
    _fused_node(fused["texels"])
    ops = chain(lambda m, r, c, l: deferred._sample_cubemap_mip_ops(m, r, c, l))
    assert torch.equal(fused["valid"], ops["valid"]) and torch.equal(fused["sampled"], ops["sampled"])
    assert torch.equal(fused["r"], ops["r"])
    assert bool(fused["sampled"].any()) and not bool(fused["sampled"].all())
    assert torch.equal(fused["sampled"], fused["valid"])
    # the statement at the fused path's own directions
    inp = dict(cubemap=env0.cpu().numpy(), directions=fused["r"].cpu().numpy()[None],
               mask=fused["covered"].cpu().numpy()[None], lod=fused["lod"].cpu().numpy()[None], lod_bias=0.0,
               seamless=True, grad=fused["g_tex"].cpu().numpy()[None])
    _, fwd, vjp = cm.statement(inp)
    assert np.array_equal(fwd["valid"][0], fused["sampled"].cpu().numpy()[..., 0])
    assert len(set(fwd["face"][fwd["valid"]].tolist())) >= 2
    assert (fwd["valid"] & (fwd["f"] == 0)).any() and (fwd["valid"] & (fwd["f"] != 0)).any()
    assert np.array_equal(_bits(fused["texels"].detach().cpu().numpy()), _bits(fwd["texels"][0]))
    r_env = _ratio(np.abs(fused["g_env"].cpu().numpy() - vjp["grad_cubemap"]), vjp["cubemap_bound"], "chain cubemap")
    levels = float(len(cm.build_chain(inp["cubemap"])) - 1)
    r_rough = _ratio(np.abs(fused["g_rough"].cpu().numpy()[None] - vjp["grad_lod"] * levels),
                     (cm.lod_bound(vjp, 3) + 2.0 ** -24 * np.abs(vjp["grad_lod"])) * levels, "chain roughness")
    scale = float(ops["g_env"].abs().max())
    d_env = float((fused["g_env"] - ops["g_env"]).abs().max()) / scale
    scale_r = float(ops["g_rough"].abs().max())
    d_rough = float((fused["g_rough"] - ops["g_rough"]).abs().max()) / scale_r
    rel_l2 = float(torch.linalg.norm(fused["g_v"] - ops["g_v"]) / torch.linalg.norm(ops["g_v"]))
    print("glossy environment chain 64x64: d loss / d cubemap %.3f of its bound (%.3g of its scale from the framework "
          "ops'), d loss / d roughness %.3f of its bound (%.3g of its scale), d loss / d world vertices rel L2 %.3g"
          % (r_env, d_env, r_rough, d_rough, rel_l2))
    assert r_env <= 1.0 and r_rough <= 1.0
    assert scale > 0 and d_env <= lighting_cases.GRAD_FRAC
    assert scale_r > 0 and d_rough <= lighting_cases.GRAD_FRAC
    assert float(fused["g_rough"][: H // 2, : W // 2].abs().max()) > 0  # (the roughness at 0 is not stuck there)
    assert bool(torch.isfinite(fused["g_v"]).all()) and float(ops["g_v"].abs().max()) > 0
    assert rel_l2 < 1e-2, rel_l2
