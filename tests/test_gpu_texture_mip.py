"""The fused mip kernels (dirt_amd/csrc/texture_mip_kernels.h through dirt_amd.deferred.build_mipmaps and
sample_texture_mip) against the numpy statement of record (tests/texture_mip_cases.py) on its whole table.

Chain, texels, valid and the saved lod: bit-exact against the float32 statement, unsampled pixels exactly 0.
grad_uv: bit-identical between two runs (a gather in a fixed order), within (C + 7) 2^-24 of its absolute terms.
grad_packed: within (n + 3) 2^-24 S per element.  grad_texture: bit-exact against a float32 restatement of the chain
gather applied to the run's own grad_packed, and end to end within sum_k W_k (n_k + 3 + L) 2^-24 S_k of the float64
vjp.  The roundings behind each bound are counted beside the bounds in texture_mip_cases.py.
Each test prints its worst measured ratio of error to bound.

Packed offsets past 2^31 elements are not exercised here: the smallest such chain (three frames of an 8192 x 8192 x 8
chain and their gradient, 17 GB, plus its statement) does not fit a test of a few seconds; every packed offset in the
kernels and the host code is formed in int64_t, checked by reading.
"""
import gc

import numpy as np
import pytest
import torch

import deferred_cases as dc
import deferred_pipeline as dp
import texture_cases as tc
import texture_mip_cases as mc
from dirt_amd import deferred

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _fused_node(y, cls):
    """y comes from the fused autograd function `cls` (directly, or through the [0] of an unbatched call)"""
    assert y.grad_fn is not None
    names = [y.grad_fn.name()] + [fn.name() for fn, _ in y.grad_fn.next_functions if fn is not None]
    assert any(cls in n for n in names), names


def _run(inp, needs=(True, True)):
    """-> dict of numpy arrays: packed, texels, valid, lod, and grad_packed, grad_texture, grad_uv (None where not
    requested)"""
    tt, ut = _gpu(inp["texture"]).requires_grad_(needs[0]), _gpu(inp["uv"]).requires_grad_(needs[1])
    mips = deferred.build_mipmaps(tt, inp["levels"])
    if needs[0]:
        _fused_node(mips.packed, "_BuildMipmapsFn")
        mips.packed.retain_grad()
    texels, valid, lod = deferred._sample_texture_mip(mips, ut, _gpu(inp["mask"]), inp["wrap"], _gpu(inp["lod"]),
                                                      inp["lod_bias"])
    assert not valid.requires_grad and not lod.requires_grad
    if any(needs):
        _fused_node(texels, "_SampleTextureMipFn")
        texels.backward(_gpu(inp["grad"]))
    torch.cuda.synchronize()
    return dict(packed=_np(mips.packed), texels=_np(texels), valid=_np(valid), lod=_np(lod), dims=mips.dims,
                grad_packed=_np(mips.packed.grad) if needs[0] else None, grad_texture=_np(tt.grad),
                grad_uv=_np(ut.grad))


def _ratio(err, bound, tag):
    """worst err / bound; where the bound is 0 the error must be"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    zero = bound == 0
    assert not np.any(err[zero]), tag
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _check_forward(got, chain, fwd, tag):
    assert list(got["dims"]) == [c.shape[-3:-1] for c in chain], tag
    assert np.array_equal(_bits(got["packed"]), _bits(mc.pack(chain))), tag
    assert got["valid"].dtype == np.bool_ and got["valid"].shape == fwd["valid"].shape + (1,), tag
    assert np.array_equal(got["valid"][..., 0], fwd["valid"]), tag
    assert np.array_equal(_bits(got["lod"]), _bits(fwd["lod"])), tag
    assert np.array_equal(_bits(got["texels"]), _bits(fwd["texels"])), tag
    assert not np.any(_bits(got["texels"])[~fwd["valid"]]), tag


def _check_grads(got, inp, vjp, tag):
    """-> worst ratios (grad_packed, grad_texture, grad_uv) of error to bound, of the gradients present"""
    rp = rt = ru = 0.0
    C = inp["texture"].shape[-1]
    if got["grad_texture"] is not None:
        Th, Tw = inp["texture"].shape[-3:-1]
        assert got["grad_packed"].shape == vjp["grad_packed"].shape, tag
        rp = _ratio(np.abs(got["grad_packed"] - vjp["grad_packed"]), mc.packed_bound(vjp), tag)
        assert rp <= 1.0, (tag, "grad_packed", rp)
        # the chain's backward: the float32 gather of the run's own grad_packed, bit for bit
        restated = mc.chain_vjp(got["grad_packed"], Th, Tw, inp["levels"], np.float32)
        assert np.array_equal(_bits(got["grad_texture"]), _bits(restated)), tag
        rt = _ratio(np.abs(got["grad_texture"] - vjp["grad_texture"]), vjp["texture_bound"], tag)
        assert rt <= 1.0, (tag, "grad_texture", rt)
    if got["grad_uv"] is not None:
        ru = _ratio(np.abs(got["grad_uv"] - vjp["grad_uv"]), mc.uv_bound(vjp, C), tag)
        assert ru <= 1.0, (tag, "grad_uv", ru)
    return rp, rt, ru


@pytest.mark.parametrize("ident", mc.CASE_IDS)
def test_matches_the_statement(ident):
    inp, chain, fwd, vjp = mc.case(ident)
    first, second = _run(inp), _run(inp)
    _check_forward(first, chain, fwd, ident)
    assert np.array_equal(_bits(first["grad_uv"]), _bits(second["grad_uv"])), ident  # no run-to-run difference
    assert not np.any(_bits(first["grad_uv"])[~fwd["valid"]]), ident
    r1, r2 = _check_grads(first, inp, vjp, ident), _check_grads(second, inp, vjp, ident)
    print("mip %s: grad_packed %.3f, grad_texture %.3f, grad_uv %.3f of their bounds"
          % (ident, max(r1[0], r2[0]), max(r1[1], r2[1]), r1[2]))


@pytest.mark.parametrize("tex,C,frames", [((64, 64), 3, 1), ((6, 10), 4, 2), ((4, 2), 1, 3), ((1, 8), 8, 1),
                                          ((96, 160), 3, 2), ((5, 7), 2, 1), ((512, 2), 5, 1),
                                          ((16, 8), 2, 2), ((8, 16), 5, 1), ((6, 10), 6, 2), ((32, 32), 7, 1)])
def test_chain_build(tex, C, frames):
    """The build's forward bit-exact; its backward on a given grad_packed bit-exact against the float32 restatement
    of the gather, identical across two runs, and it leaves the incoming gradient as it was."""
    rng = np.random.default_rng(tex[0] * 7 + tex[1] + C)
    texture = rng.standard_normal((frames,) + tex + (C,)).astype(np.float32)
    chain = mc.build_chain(texture)
    gp = rng.standard_normal(mc.pack(chain).shape).astype(np.float32)
    want = mc.chain_vjp(gp, tex[0], tex[1], None, np.float32)
    grads = []
    for _ in range(2):
        tt, g = _gpu(texture).requires_grad_(True), _gpu(gp)
        mips = deferred.build_mipmaps(tt)
        assert len(mips) == len(chain) and np.array_equal(_bits(_np(mips.packed)), _bits(mc.pack(chain)))
        mips.packed.backward(g)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_np(g)), _bits(gp))
        grads.append(_np(tt.grad))
    assert np.array_equal(_bits(grads[0]), _bits(want)) and np.array_equal(_bits(grads[0]), _bits(grads[1]))
    # truncated, unbatched
    tt = _gpu(texture[0]).requires_grad_(True)
    mips = deferred.build_mipmaps(tt, levels=2)
    short = mc.build_chain(texture[0], 2)
    assert len(mips) == len(short) and np.array_equal(_bits(_np(mips.packed)), _bits(mc.pack(short)))
    g2 = gp[0, :mips.packed.shape[0]]
    mips.packed.backward(_gpu(g2))
    assert np.array_equal(_bits(_np(tt.grad)), _bits(mc.chain_vjp(g2, tex[0], tex[1], 2, np.float32)))


@pytest.mark.parametrize("kind,C,frames", [("magnify", 3, 1), ("scatter", 3, 1), ("magnify", 8, 2), ("scatter", 4, 2)]
                         + [(kind, C, 1) for C in (2, 5, 6, 7) for kind in ("magnify", "scatter")])
def test_exact_scatter(kind, C, frames):
    """Coordinates on half texels of every level read, f in {0, 1/2}, small integer cotangents: every product and
    partial sum is exact in float32, so grad_packed and grad_texture equal the statement exactly whatever the order
    of the atomics -- many pixels per texel (magnify), spread over the texture (scatter), summed over the frames."""
    inp, chain, fwd, vjp = mc.exact_scatter_case(kind, C, frames)
    got = _run(inp)
    _check_forward(got, chain, fwd, kind)
    assert np.array_equal(got["grad_packed"].astype(np.float64), vjp["grad_packed"]), kind
    assert np.array_equal(got["grad_texture"].astype(np.float64), vjp["grad_texture"]), kind
    assert np.count_nonzero(vjp["grad_texture"]) > 0
    _check_grads(got, inp, vjp, kind)


@pytest.mark.parametrize("wrap", ["clamp", "repeat"])
@pytest.mark.parametrize("kind,C,frames", [("magnify16", 3, 1), ("scatter", 8, 2)])
def test_one_level_is_sample_texture(kind, C, frames, wrap):
    """The GPU form of test_texture_mip_cpu.py's test of this name, and the pin of what the two headers share: over a
    one-level chain the mip kernels are the plain kernels' per-level functions called once, so texels, valid, grad_uv
    and grad_texture equal sample_texture's bit for bit, every element -- with the lod taken from the uv differences,
    and with an explicit random lod and a lod_bias (both clamp to level 0).  texture_cases.exact_scatter_case: every
    product and partial sum is exact in float32, so the order of the atomics cannot excuse a difference; magnify16
    goes through both kernels' LDS patches, scatter through their direct atomics."""
    (texture, uv, mask, _, grad), fwd, vjp = tc.exact_scatter_case(kind, C, frames)
    assert uv.shape == (frames, 63, 65, 2) and texture.shape == (64, 64, C)
    assert np.count_nonzero(vjp["grad_texture"]) > 0 and np.count_nonzero(vjp["grad_uv"]) > 0

    def run(sample):
        tt, ut = _gpu(texture).requires_grad_(True), _gpu(uv).requires_grad_(True)
        texels, valid = sample(tt, ut)
        texels.backward(_gpu(grad))
        torch.cuda.synchronize()
        return dict(texels=_np(texels), valid=_np(valid), grad_uv=_np(ut.grad), grad_texture=_np(tt.grad))

    def plain(tt, ut):
        texels, valid = deferred.sample_texture(tt, ut, _gpu(mask), wrap)
        _fused_node(texels, "_SampleTextureFn")
        return texels, valid

    want = run(plain)
    assert want["valid"].any() and not want["valid"].all()
    rng = np.random.default_rng(20)
    for lod, lod_bias in ((None, 0.0), (rng.uniform(-3.0, 9.0, uv.shape[:-1]).astype(np.float32), 0.75)):
        def mip(tt, ut):
            mips = deferred.build_mipmaps(tt, levels=1)
            assert len(mips) == 1
            texels, valid = deferred.sample_texture_mip(mips, ut, _gpu(mask), wrap, _gpu(lod), lod_bias)
            _fused_node(texels, "_SampleTextureMipFn")
            return texels, valid

        got = run(mip)
        for name in ("texels", "grad_uv", "grad_texture"):
            assert got[name].shape == want[name].shape, (name, lod_bias)
            assert np.array_equal(_bits(got[name]), _bits(want[name])), (name, lod_bias)
        assert got["valid"].dtype == np.bool_ and np.array_equal(got["valid"], want["valid"]), lod_bias


def test_integer_lod_does_not_read_the_next_level():
    """Every pixel at lod 1 exactly, over a hand-made chain whose levels 0 and 2 hold NaN and inf: output and
    gradients are finite and equal the statement's on the clean chain, levels 0 and 2 receive no gradient."""
    inp = dict(mc.case_input("17x33-t64x64-c3-shared-min2-clamp-frac-bg"))
    shape = inp["uv"].shape[:-1]
    inp["lod"], inp["lod_bias"] = np.ones(shape, np.float32), 0.0
    chain, fwd, vjp = mc.statement(inp)
    assert fwd["valid"].any() and set(fwd["levels"]) == {1}
    dims, offs, n = mc.layout(64, 64)
    packed = _gpu(mc.pack(chain))
    packed[offs[0]:offs[1]] = float("nan")
    packed[offs[2]:offs[3]] = float("inf")
    packed.requires_grad_(True)
    ut = _gpu(inp["uv"]).requires_grad_(True)
    texels, valid = deferred.sample_texture_mip(deferred.Mipmaps(packed, 64, 64), ut, None, "clamp", _gpu(inp["lod"]))
    _fused_node(texels, "_SampleTextureMipFn")
    texels.backward(_gpu(inp["grad"]))
    assert np.array_equal(_bits(_np(texels)), _bits(fwd["texels"]))
    gp, gu = _np(packed.grad), _np(ut.grad)
    assert np.all(np.isfinite(gp)) and np.all(np.isfinite(gu))
    assert not np.any(gp[offs[0]:offs[1]]) and not np.any(gp[offs[2]:])
    assert _ratio(np.abs(gp - vjp["grad_packed"]), mc.packed_bound(vjp), "planted") <= 1.0
    assert _ratio(np.abs(gu - vjp["grad_uv"]), mc.uv_bound(vjp, 3), "planted") <= 1.0


@pytest.mark.parametrize("needs", [(False, False), (True, False), (False, True)], ids=["none", "texture", "uv"])
def test_gradient_subsets(needs):
    ident = "17x33-t64x64-c4-shared-zoom-clamp-auto-bg"
    inp, chain, fwd, vjp = mc.case(ident)
    got, full = _run(inp, needs), _run(inp)
    _check_forward(got, chain, fwd, ident)
    assert (got["grad_texture"] is not None) == needs[0] and (got["grad_uv"] is not None) == needs[1]
    _check_grads(got, inp, vjp, "subset %s" % (needs,))
    if needs[1]:
        assert np.array_equal(_bits(got["grad_uv"]), _bits(full["grad_uv"]))
    if needs[0]:
        assert np.all(np.abs(got["grad_texture"] - full["grad_texture"]) <= 2 * vjp["texture_bound"])


def test_forms(monkeypatch):
    """[H,W,2] with a shared chain, a plain texture in place of the chain, non-contiguous views, bool and integer
    masks, a float64 lod run the fused kernels; float64 operands and DIRT_FUSED_DEFERRED=0 take the statement, with no
    fused node."""
    ident = "17x33-t64x64-c3-shared-min2-clamp-frac-bg"
    inp = dict(mc.case_input(ident))
    inp["mask"] = (np.isfinite(inp["uv"]).all(-1) & (np.random.default_rng(2).random(inp["uv"].shape[:-1]) < 0.7)
                   ).astype(np.uint8)
    chain, fwd, vjp = mc.statement(inp)
    base = _run(inp)
    _check_forward(base, chain, fwd, ident)
    _check_grads(base, inp, vjp, ident)
    # unbatched, a plain texture, bool mask, float64 lod
    tt, ut = _gpu(inp["texture"]).requires_grad_(True), _gpu(inp["uv"][0]).requires_grad_(True)
    texels, valid = deferred.sample_texture_mip(tt, ut, _gpu(inp["mask"][0]).bool(), "clamp",
                                                _gpu(inp["lod"][0]).double())
    _fused_node(texels, "_SampleTextureMipFn")
    assert texels.shape == (17, 33, 3) and valid.shape == (17, 33, 1) and valid.dtype == torch.bool
    texels.backward(_gpu(inp["grad"][0]))
    assert np.array_equal(_bits(_np(texels)), _bits(base["texels"][0]))
    assert np.array_equal(_bits(_np(ut.grad)), _bits(base["grad_uv"][0]))
    assert np.all(np.abs(_np(tt.grad) - vjp["grad_texture"]) <= vjp["texture_bound"])
    # non-contiguous views, integer mask
    wide_t, wide_u = torch.zeros((64, 64, 6), device=DEV), torch.zeros((1, 17, 33, 4), device=DEV)
    wide_t[..., ::2], wide_u[..., ::2] = _gpu(inp["texture"]), _gpu(inp["uv"])
    wide_t.requires_grad_(True), wide_u.requires_grad_(True)
    texels, valid = deferred.sample_texture_mip(wide_t[..., ::2], wide_u[..., ::2], _gpu(inp["mask"]).long(), "clamp",
                                                _gpu(inp["lod"]))
    _fused_node(texels, "_SampleTextureMipFn")
    texels.backward(_gpu(inp["grad"]))
    assert np.array_equal(_bits(_np(texels)), _bits(base["texels"]))
    assert np.array_equal(_bits(_np(wide_u.grad)[..., ::2]), _bits(base["grad_uv"]))
    assert float(wide_u.grad[..., 1::2].abs().max()) == 0.0 and float(wide_t.grad[..., 1::2].abs().max()) == 0.0
    assert np.all(np.abs(_np(wide_t.grad)[..., ::2] - vjp["grad_texture"]) <= vjp["texture_bound"])
    # a per-frame chain on a batch
    ident_b = "3x5x6-t64x64-c3-perframe-min2-clamp-frac-bg"
    inp_b, chain_b, fwd_b, vjp_b = mc.case(ident_b)
    got_b = _run(inp_b)
    assert got_b["packed"].shape == (3, mc.layout(64, 64)[2], 3)
    _check_forward(got_b, chain_b, fwd_b, ident_b)
    _check_grads(got_b, inp_b, vjp_b, ident_b)
    # float64 and the switch: the framework-op statement
    f64 = mc.statement(inp, np.float64)[1]
    t64 = _gpu(inp["texture"]).double().requires_grad_(True)
    y64, _ = deferred.sample_texture_mip(t64, _gpu(inp["uv"]).double(), _gpu(inp["mask"]), "clamp", _gpu(inp["lod"]))
    assert "_SampleTextureMipFn" not in y64.grad_fn.name()
    assert np.abs(_np(y64) - f64["texels"]).max() <= 1e-12
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    tt = _gpu(inp["texture"]).requires_grad_(True)
    mips = deferred.build_mipmaps(tt)
    assert "_BuildMipmapsFn" not in mips.packed.grad_fn.name()
    y, v = deferred.sample_texture_mip(mips, _gpu(inp["uv"]), _gpu(inp["mask"]), "clamp", _gpu(inp["lod"]))
    assert "_SampleTextureMipFn" not in y.grad_fn.name()
    assert np.array_equal(_np(v)[..., 0], fwd["valid"])
    # (two roundings per chain level, four inside a level and two for the blend on any path from a texel to the output,
    # whatever the framework's kernels contract)
    assert np.abs(_np(y) - fwd["texels"]).max() <= (2 * 6 + 4 + 2 + 1) * 2.0 ** -24 * np.abs(inp["texture"]).max()


def test_fused_backward_refuses_double_backward(monkeypatch):
    inp = mc.case_input("16x16-t64x64-c3-shared-min2-repeat-auto")
    tt, ut = _gpu(inp["texture"]).requires_grad_(True), _gpu(inp["uv"]).requires_grad_(True)
    texels, _ = deferred.sample_texture_mip(tt, ut)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(texels.square().sum(), [ut], create_graph=True)
    mips = deferred.build_mipmaps(tt)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(mips.packed.square().sum(), [tt], create_graph=True)
    monkeypatch.setattr(deferred, "_FUSED_ENABLED", False)
    texels, _ = deferred.sample_texture_mip(tt, ut)
    g, = torch.autograd.grad(texels.square().sum(), [ut], create_graph=True)
    gg, = torch.autograd.grad(g.square().sum(), [tt])
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().sum()) > 0


def test_captures_into_a_graph():
    """Chain build, lookup and both backwards captured with torch.cuda.graph on one stream (no parallel branches; the
    zero-fill of grad_packed is an asynchronous memset on it), replayed after uv and texture changed in place: equal
    to the eager result, grad_uv bit for bit, the texture gradient within the bound."""
    first = mc.case_input("17x33-t64x64-c3-shared-min2-repeat-auto")
    second = dict(first, wrap="clamp")  # the same shapes: a re-seeded texture under the zooming warp
    second["texture"] = np.random.default_rng(21).standard_normal(first["texture"].shape).astype(np.float32)
    second["uv"] = np.ascontiguousarray(mc._uv_zoom((1, 17, 33), 64, 64, None), np.float32)
    chain2, fwd2, vjp2 = mc.statement(second)
    assert fwd2["valid"].all() and len(set(np.unique(fwd2["k0"]))) >= 3
    tt, ut = _gpu(first["texture"]).requires_grad_(True), _gpu(first["uv"]).requires_grad_(True)
    g = _gpu(second["grad"])
    out = {}

    def step():
        texels, valid, lod = deferred._sample_texture_mip(tt, ut)
        out["texels"], out["valid"], out["lod"] = texels, valid, lod
        out["grads"] = torch.autograd.grad(texels, [tt, ut], g)

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
        tt.copy_(_gpu(second["texture"]))
        ut.copy_(_gpu(second["uv"]))
    graph.replay()
    torch.cuda.synchronize()
    got = dict(texels=_np(out["texels"]), valid=_np(out["valid"]), lod=_np(out["lod"]),
               grad_texture=_np(out["grads"][0]), grad_uv=_np(out["grads"][1]))
    del graph
    out.clear()
    eager = _run(second)
    assert np.array_equal(_bits(got["texels"]), _bits(fwd2["texels"])) and np.array_equal(got["valid"], eager["valid"])
    assert np.array_equal(_bits(got["lod"]), _bits(fwd2["lod"]))
    assert np.array_equal(_bits(got["texels"]), _bits(eager["texels"]))
    assert np.array_equal(_bits(got["grad_uv"]), _bits(eager["grad_uv"]))
    rt = _ratio(np.abs(got["grad_texture"] - vjp2["grad_texture"]), vjp2["texture_bound"], "graph")
    ru = _ratio(np.abs(got["grad_uv"] - vjp2["grad_uv"]), mc.uv_bound(vjp2, 3), "graph")
    print("graph replay: grad_texture %.3f of its bound, grad_uv %.3f of its bound" % (rt, ru))
    assert rt <= 1.0 and ru <= 1.0


def test_chain_textured_deferred_shading():
    """The deferred chain of tests/test_gpu_texture.py's textured test with a 64 x 64 x 3 texture, seen at about 2x
    minification by the 64 x 64 frame (uv = x / 2.15 + 0.5, 2.6 y + 0.5: the median lod of the sampled pixels is about
    1, and the uv leaves [0, 1] a little at the rim, where it clamps): uv rendered over -inf, dilated, looked up by
    the fused sample_texture_mip, shaded.  Against the framework-op lookup on the GPU, everything else shared: valid
    equal; pixels within the shade's forward contract.  Against the numpy statement on the fused path's own uv
    buffer and colour cotangent: colours and lod bit for bit, d loss / d texture within the end-to-end bound.  The
    distances to the framework ops' gradients (d loss / d texture over its scale, d loss / d world vertices in
    relative L2) are printed, not asserted: no bound is derived for them."""
    H = W = 64
    world, faces, albedo = dp.grid_surface(n=12)
    f, al = _gpu(faces), _gpu(albedo)
    wts = torch.rand((H, W, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    tex0 = torch.rand((64, 64, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 0.8 + 0.2
    grey, ld, red, white = dp._constants(DEV)
    cam = dp.camera_position(H, W, DEV)
    ninf2 = torch.full((H, W, 2), float("-inf"), device=DEV)

    def chain(lookup):
        Vw, tex = _gpu(world).requires_grad_(True), tex0.clone().requires_grad_(True)
        pos, _, nrm, clip = dp.gbuffers(dp.hip_render, Vw, f, al, H, W)
        vertex_uv = torch.stack([Vw[:, 0] / 2.15 + 0.5, Vw[:, 1] * 2.6 + 0.5], -1)
        uvbuf = deferred.dilate(dp.hip_render(ninf2, clip, vertex_uv, f, H, W, 2))
        colours, sampled, lod = lookup(tex, uvbuf)
        pixels, valid = deferred.shade(pos, colours, nrm, grey, ld, red, white, cam, 6., False)
        g_tex, g_v = torch.autograd.grad(dp.loss_fn(pixels, valid, wts), [tex, Vw], retain_graph=True)
        g_col, = torch.autograd.grad(dp.loss_fn(pixels, valid, wts), [colours])
        return dict(pixels=pixels.detach(), valid=valid, sampled=sampled, colours=colours, uvbuf=uvbuf.detach(),
                    g_tex=g_tex, g_v=g_v, g_col=g_col, pos=pos.detach(), nrm=nrm.detach(), lod=lod)

    fused = chain(lambda t, u: deferred._sample_texture_mip(t, u))
    _fused_node(fused["colours"], "_SampleTextureMipFn")
    ops = chain(lambda t, u: deferred._sample_texture_mip_ops(deferred._build_mipmaps_ops(t), u))
    assert torch.equal(fused["valid"], ops["valid"]) and torch.equal(fused["sampled"], ops["sampled"])
    assert bool(fused["valid"].any()) and not bool(fused["valid"].all()) and bool(fused["sampled"].any())
    lod = fused["lod"][fused["sampled"][..., 0]]
    print("textured mip chain: lod min %.3f median %.3f max %.3f" % (float(lod.min()), float(lod.median()),
                                                                     float(lod.max())))
    assert 0.75 <= float(lod.median()) <= 1.25  # (about 2x minification: lod 1)
    L = dc.Lights(camera=cam.cpu().numpy())
    L.ambient, L.direction, L.diffuse, L.specular = (t.cpu().numpy() for t in (grey, ld, red, white))
    ref = dc.shade(_np(ops["pos"]), _np(ops["colours"]), _np(ops["nrm"]), L)
    r_px = _ratio(_np((fused["pixels"] - ops["pixels"]).abs()), dc.shade_fwd_bound(ref), "chain pixels")
    inp = dict(texture=_np(tex0), uv=_np(fused["uvbuf"])[None], mask=None, wrap="clamp", lod=None, lod_bias=0.0,
               levels=None, grad=_np(fused["g_col"])[None])
    _, fwd, vjp = mc.statement(inp)
    assert np.array_equal(fwd["valid"][0], _np(fused["sampled"])[..., 0])
    assert np.array_equal(_bits(_np(fused["lod"])), _bits(fwd["lod"][0]))
    assert np.array_equal(_bits(_np(fused["colours"])), _bits(fwd["texels"][0]))
    r_tex = _ratio(np.abs(_np(fused["g_tex"]) - vjp["grad_texture"]), vjp["texture_bound"], "chain texture")
    scale = float(ops["g_tex"].abs().max())
    d_tex = float((fused["g_tex"] - ops["g_tex"]).abs().max()) / scale
    rel_l2 = float(torch.linalg.norm(fused["g_v"] - ops["g_v"]) / torch.linalg.norm(ops["g_v"]))
    print("textured mip chain 64x64: pixels %.3f of the bound, d loss / d texture %.3f of the end-to-end bound (%.3g "
          "of its scale from the framework ops'), d loss / d world vertices rel L2 %.3g" % (r_px, r_tex, d_tex, rel_l2))
    assert r_px <= 1.0 and r_tex <= 1.0
    assert scale > 0 and bool(torch.isfinite(fused["g_v"]).all()) and float(ops["g_v"].abs().max()) > 0
