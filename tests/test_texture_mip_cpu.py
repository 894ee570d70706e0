"""dirt_amd.deferred.build_mipmaps / sample_texture_mip on a CPU: the host-only layout entry point and the framework-op
statements (`_build_mipmaps_ops`, `_sample_texture_mip_ops`) against the numpy statement of record
(tests/texture_mip_cases.py) on its whole table, float64 anchors that share no code with the project (avg_pool2d, an
affine texture, grid_sample + lerp), the one-level chain against sample_texture, and the argument checks of the
public entries and of the C entry points (no GPU call is made).
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import texture_cases as tc
import texture_mip_cases as mc
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_texture_mip_layout", "dirt_texture_mip_build_fwd", "dirt_texture_mip_build_bwd",
               "dirt_texture_sample_mip_fwd", "dirt_texture_sample_mip_bwd")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _t(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _ratio(err, bound, tag):
    """worst err / bound; where the bound is 0 the error must be"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    zero = bound == 0
    assert not np.any(err[zero]), tag
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _c_layout(Th, Tw, max_levels):
    dims = (ctypes.c_int * (2 * _lib.MAX_MIP_LEVELS))()
    offs = (ctypes.c_longlong * _lib.MAX_MIP_LEVELS)()
    total = ctypes.c_longlong(-1)
    L = _lib.load().dirt_texture_mip_layout(Th, Tw, max_levels, dims, offs, ctypes.byref(total))
    return L, [(dims[2 * k], dims[2 * k + 1]) for k in range(L)], list(offs[:L]), total.value


@pytest.mark.parametrize("tex", mc.TEXTURES + [(8192, 8192), (8192, 1), (1, 8192), (6, 10), (4096, 6), (96, 160)])
def test_layout_entry_point(tex):
    full = mc.layout(*tex)
    for levels in (None, 1, 2, 3, len(full[0]), len(full[0]) + 5):
        dims, offs, n = mc.layout(tex[0], tex[1], levels)
        assert _c_layout(tex[0], tex[1], levels or 0) == (len(dims), dims, offs, n), (tex, levels)
        assert deferred._mip_dims(tex[0], tex[1], levels) == dims
    assert _c_layout(tex[0], tex[1], -3)[0] == len(full[0])
    assert _lib.load().dirt_texture_mip_layout(tex[0], tex[1], 0, None, None, None) == len(full[0])


def test_layout_examples():
    assert [len(mc.layout(*t)[0]) for t in ((5, 7), (6, 10), (64, 64), (8192, 8192), (4, 2), (1, 8), (1, 1))] == \
        [1, 2, 7, 14, 3, 4, 1]
    assert _lib.MAX_MIP_LEVELS == 14
    assert mc.layout(4, 2)[0] == [(4, 2), (2, 1), (1, 1)] and mc.layout(6, 10)[0] == [(6, 10), (3, 5)]
    lib = _lib.load()
    for bad in ((0, 4), (4, 0), (_lib.MAX_DIM + 1, 4), (4, -1)):
        assert lib.dirt_texture_mip_layout(bad[0], bad[1], 0, None, None, None) == 0
        assert "texture height, width" in lib.dirt_last_error().decode()


def _mipmaps(inp, dtype=None, leaf=False):
    tt = _t(inp["texture"], dtype).requires_grad_(leaf)
    return tt, deferred._build_mipmaps_ops(tt, inp["levels"])


@pytest.mark.parametrize("ident", mc.CASE_IDS)
def test_ops_match_the_statement(ident):
    """float32 on a CPU: the chain, texels, valid and the lod bit for bit, unsampled pixels exactly 0; the public
    entries take the same route."""
    inp, chain, fwd, _ = mc.case(ident)
    _, mips = _mipmaps(inp)
    assert list(mips.dims) == [c.shape[-3:-1] for c in chain] and len(mips) == len(chain)
    assert np.array_equal(_bits(mips.packed.numpy()), _bits(mc.pack(chain))), ident
    for k in range(len(chain)):
        assert np.array_equal(_bits(mips.level(k).numpy()), _bits(chain[k])), (ident, k)
    texels, valid, lod = deferred._sample_texture_mip_ops(mips, _t(inp["uv"]), _t(inp["mask"]), inp["wrap"],
                                                          _t(inp["lod"]), inp["lod_bias"])
    assert valid.dtype == torch.bool and tuple(valid.shape) == inp["uv"].shape[:-1] + (1,)
    assert np.array_equal(valid.numpy()[..., 0], fwd["valid"]), ident
    assert np.array_equal(_bits(lod.numpy()), _bits(fwd["lod"])), ident
    assert np.array_equal(_bits(texels.numpy()), _bits(fwd["texels"])), ident
    assert not np.any(_bits(texels.numpy())[~fwd["valid"]]), ident
    pub_m = deferred.build_mipmaps(_t(inp["texture"]), inp["levels"])
    assert isinstance(pub_m, deferred.Mipmaps) and torch.equal(pub_m.packed, mips.packed)
    pub = deferred.sample_texture_mip(pub_m, _t(inp["uv"]), _t(inp["mask"]), inp["wrap"], _t(inp["lod"]),
                                      inp["lod_bias"])
    assert len(pub) == 2 and np.array_equal(_bits(pub[0].numpy()), _bits(fwd["texels"])) and torch.equal(pub[1], valid)


# (a case without a sampled pixel has no gradient to check: test_ops_match_the_statement covers its forward)
SAMPLED_IDS = [i for i in mc.CASE_IDS if mc.case(i)[2]["valid"].any()]
assert 0 < len(mc.CASE_IDS) - len(SAMPLED_IDS) < 10


@pytest.mark.parametrize("ident", SAMPLED_IDS)
def test_ops_autograd_within_the_bounds(ident):
    """The framework statement's autograd against the float64 vjp.  In float64 (the statement evaluated in float64 on
    the same inputs): within 1e-12 of each gradient's scale.  In float32: grad_packed, the end-to-end grad_texture
    and grad_uv within the statement's bounds of the float64 vjp of the float32 forward."""
    inp, chain, fwd, vjp = mc.case(ident)
    C = inp["texture"].shape[-1]
    # float64
    chain64, fwd64, vjp64 = mc.statement(inp, np.float64)
    tt, mips = _mipmaps(inp, torch.float64, leaf=True)
    ut = _t(inp["uv"], torch.float64).requires_grad_(True)
    lt = None if inp["lod"] is None else _t(inp["lod"], torch.float64).requires_grad_(True)
    texels, valid, _ = deferred._sample_texture_mip_ops(mips, ut, _t(inp["mask"]), inp["wrap"], lt, inp["lod_bias"])
    assert not valid.requires_grad
    assert np.abs(texels.detach().numpy() - fwd64["texels"]).max() <= 1e-12 * max(1.0, np.abs(fwd64["texels"]).max())
    gt, gu = torch.autograd.grad(texels, [tt, ut], _t(inp["grad"], torch.float64), retain_graph=True)
    for name, got in (("grad_texture", gt), ("grad_uv", gu)):
        got = got.numpy()
        assert np.all(np.isfinite(got)), (ident, name)
        assert np.abs(got - vjp64[name]).max() <= 1e-12 * max(1.0, np.abs(vjp64[name]).max()), (ident, name)
    assert not np.any(gu.numpy()[~fwd["valid"]])
    if lt is not None:  # the lod carries no gradient
        assert torch.autograd.grad(texels, [lt], _t(inp["grad"], torch.float64), allow_unused=True)[0] is None
    # float32
    tt, mips = _mipmaps(inp, leaf=True)
    packed = mips.packed
    ut = _t(inp["uv"]).requires_grad_(True)
    texels, _, _ = deferred._sample_texture_mip_ops(mips, ut, _t(inp["mask"]), inp["wrap"], _t(inp["lod"]),
                                                    inp["lod_bias"])
    gp, gt, gu = torch.autograd.grad(texels, [packed, tt, ut], _t(inp["grad"]))
    rp = _ratio(np.abs(gp.numpy() - vjp["grad_packed"]), mc.packed_bound(vjp), ident)
    rt = _ratio(np.abs(gt.numpy() - vjp["grad_texture"]), vjp["texture_bound"], ident)
    ru = _ratio(np.abs(gu.numpy() - vjp["grad_uv"]), mc.uv_bound(vjp, C), ident)
    print("mip ops %s: grad_packed %.3f, grad_texture %.3f, grad_uv %.3f of their bounds" % (ident, rp, rt, ru))
    assert rp <= 1.0 and rt <= 1.0 and ru <= 1.0, (ident, rp, rt, ru)


@pytest.mark.parametrize("wrap", tc.WRAPS)
def test_one_level_is_sample_texture(wrap):
    """5 x 7 has one level: whatever the uv differences, an explicit lod or the bias say, the lookup is sample_texture
    bit for bit (values and the texture gradient; the uv gradient within texture_cases' bound)."""
    (texture, uv, mask, _, grad), fwd, _ = tc.case("63x65-t5x7-c8-shared-random-clamp-bg")
    assert len(mc.layout(5, 7)[0]) == 1 and 0.1 < fwd["valid"].mean() < 0.9
    rng = np.random.default_rng(5)
    for lod, bias in ((None, 0.0), (None, 2.5), (rng.uniform(-3, 3, uv.shape[:-1]).astype(np.float32), -0.5)):
        tt, ut = _t(texture).requires_grad_(True), _t(uv).requires_grad_(True)
        ref, ref_valid = deferred.sample_texture(tt, ut, _t(mask), wrap)
        got, valid = deferred.sample_texture_mip(tt, ut, _t(mask), wrap, _t(lod), bias)
        assert torch.equal(valid, ref_valid)
        assert np.array_equal(_bits(got.detach().numpy()), _bits(ref.detach().numpy()))
        (gt, gu), (rt, ru) = torch.autograd.grad(got, [tt, ut], _t(grad)), torch.autograd.grad(ref, [tt, ut], _t(grad))
        assert np.array_equal(_bits(gt.numpy()), _bits(rt.numpy()))
        # (the uv gradient of the mip statement rounds texel differences, as the kernels and the statement's bound do,
        # where sample_texture's framework ops round differences of products: the same number, not the same bits --
        # DESIGN 6c)
        vjp = tc.sample_vjp(texture, grad, tc.sample(texture, uv, mask, wrap))
        assert np.all(np.abs(gu.numpy() - vjp["grad_uv"]) <= tc.uv_bound(vjp, 8))
        assert not np.any(gu.numpy()[~fwd["valid"]]) and np.array_equal(gu.numpy() == 0, ru.numpy() == 0)


def _kink_free(rng, shape):
    """(uv float64 [shape,2], lod) over an 8 x 8 chain: texel coordinates 2 m + 1.2 + d at level 0 and m + 0.35 + d / 2
    at level 1, d in [0, 0.5] -- inside a texel cell at both levels, inside (0, 1), away from every kink of the rule"""
    m = rng.integers(0, 3, shape + (2,))
    x0 = 2 * m + 1.2 + rng.uniform(0.0, 0.5, shape + (2,))
    return torch.from_numpy((x0 + 0.5) / 8.0), torch.from_numpy(rng.uniform(0.2, 0.8, shape))


@pytest.mark.parametrize("wrap", tc.WRAPS)
def test_second_derivatives_of_the_ops(wrap):
    """The framework statement differentiates twice (it is where the fused backward's refusal sends a caller): float64,
    away from the kinks.  torch.autograd.gradgradcheck over texture and uv at a fractional lod; d(grad_uv) / d(uv)
    against central differences, its mixed u-v entry nonzero; and with one level, every second derivative equal to
    sample_texture's."""
    rng = np.random.default_rng(17)
    uv, lod = _kink_free(rng, (2, 3))
    texture = torch.from_numpy(rng.standard_normal((8, 8, 2)))
    g = torch.from_numpy(rng.standard_normal((2, 3, 2)))

    def lookup(t, u, levels=None):
        return deferred._sample_texture_mip_ops(deferred._build_mipmaps_ops(t, levels), u, None, wrap, lod)[0]

    t_, u_ = texture.clone().requires_grad_(True), uv.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lookup, (t_, u_), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradgradcheck(lookup, (t_, u_), eps=1e-6, atol=1e-6)

    def grad_uv(u):
        u = u.clone().requires_grad_(True)
        return torch.autograd.grad(lookup(texture, u), [u], g, create_graph=True)[0], u

    gu, u = grad_uv(uv)
    for comp in (0, 1):  # d grad_uv[1, 1, comp] / d uv[1, 1, :]: the mixed entry is the off-diagonal one
        hess = torch.autograd.grad(gu[1, 1, comp], [u], retain_graph=True)[0][1, 1]
        for k in (0, 1):
            e = torch.zeros_like(uv)
            e[1, 1, k] = 1e-6
            fd = (grad_uv(uv + e)[0][1, 1, comp] - grad_uv(uv - e)[0][1, 1, comp]).detach() / 2e-6
            assert abs(float(hess[k] - fd)) <= 1e-6 * max(1.0, abs(float(fd))), (comp, k, float(hess[k]), float(fd))
        assert float(hess[comp]) == 0.0 and abs(float(hess[1 - comp])) > 1e-3  # (bilinear in u, v: only the mixed term)
    # one level: sample_texture's second derivatives
    loss = lambda y: (y * g).sum().square() + y.square().sum()  # noqa: E731
    seconds = []
    for fn in (lambda t, u: lookup(t, u, 1), lambda t, u: deferred._sample_texture_ops(t, u, None, wrap)[0]):
        t_, u_ = texture.clone().requires_grad_(True), uv.clone().requires_grad_(True)
        gt1, gu1 = torch.autograd.grad(loss(fn(t_, u_)), [t_, u_], create_graph=True)
        seconds.append(torch.autograd.grad(gu1.sin().sum() + gt1.cos().sum(), [t_, u_]))
    for a, b in zip(*seconds):
        assert float(b.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())


@pytest.mark.parametrize("tex", [(2, 2), (8, 8), (6, 10), (64, 64), (4, 2), (1, 8), (96, 160)])
def test_chain_is_avg_pool2d(tex):
    """float64: every level whose parent has both dimensions >= 2 is avg_pool2d(2) of it; a level under a parent with
    a dimension of 1 is the mean of its pairs (avg_pool1d)."""
    rng = np.random.default_rng(tex[0] * 31 + tex[1])
    texture = torch.from_numpy(rng.standard_normal((2,) + tex + (3,)))
    mips = deferred.build_mipmaps(texture)
    assert len(mips) == len(mc.layout(*tex)[0]) and mips.packed.shape == (2, mc.layout(*tex)[2], 3)
    for k in range(1, len(mips)):
        parent = mips.level(k - 1).permute(0, 3, 1, 2)
        h, w = mips.dims[k - 1]
        if h >= 2 and w >= 2:
            ref = Fn.avg_pool2d(parent, 2)
        else:
            ref = Fn.avg_pool1d(parent.reshape(2, 3, h * w), 2).reshape((2, 3) + mips.dims[k])
        assert float((mips.level(k).permute(0, 3, 1, 2) - ref).abs().max()) <= 1e-15, (tex, k)
    assert np.abs(mc.pack(mc.build_chain(texture.numpy(), None, np.float64)) - mips.packed.numpy()).max() <= 1e-15


def test_levels_are_aligned():
    """A texture affine in the texel centres' (u, v), looked up in clamp mode away from the border, returns the affine
    value at any lod (the box filter and the bilinear rule both preserve affine functions; a level shifted by half a
    texel would not), to 1e-12 in float64 -- and so do the automatic lod and a bias."""
    rng = np.random.default_rng(11)
    Th, Tw = 64, 32
    i, j = np.meshgrid(np.arange(Th), np.arange(Tw), indexing="ij")
    coef = rng.standard_normal((3, 2))
    texture = coef[0] + coef[1] * ((j[..., None] + 0.5) / Tw) + coef[2] * ((i[..., None] + 0.5) / Th)
    uv = rng.uniform(0.3, 0.7, (2, 9, 11, 2))  # level 3 is 8 x 4: its border band ends at u = 1/8, v = 1/16
    want = coef[0] + coef[1] * uv[..., :1] + coef[2] * uv[..., 1:]
    mips = deferred.build_mipmaps(torch.from_numpy(texture), levels=4)
    for lod, bias in ((rng.uniform(0, 3, uv.shape[:-1]), 0.0), (np.full(uv.shape[:-1], 1.5), 0.25), (None, 0.0),
                      (None, -2.0)):
        got, valid = deferred.sample_texture_mip(mips, torch.from_numpy(uv), None, "clamp", _t(lod), bias)
        assert bool(valid.all())
        assert np.abs(got.numpy() - want).max() <= 1e-12, (bias, np.abs(got.numpy() - want).max())


@pytest.mark.parametrize("tex", [(8, 8), (6, 10), (64, 64), (4, 2)])
def test_trilinear_is_grid_sample_and_a_lerp(tex):
    """float64, clamp mode, a given lod: each level by grid_sample(bilinear, border, align_corners=False) over an
    avg_pool2d chain, then a lerp; values, d/dtexture and d/duv."""
    rng = np.random.default_rng(tex[0] * 100 + tex[1])
    B, H, W, C = 2, 7, 9, 3
    L = len(mc.layout(*tex)[0])
    texture = torch.from_numpy(rng.standard_normal((B,) + tex + (C,))).requires_grad_(True)
    uv = torch.from_numpy(rng.uniform(-0.2, 1.2, (B, H, W, 2))).requires_grad_(True)
    lod = torch.from_numpy(rng.uniform(0, L - 1, (B, H, W)))
    lod[0, 0, :3] = torch.tensor([0.0, float(L - 1), float(min(1, L - 1))])
    g = torch.from_numpy(rng.standard_normal((B, H, W, C)))
    got, valid = deferred.sample_texture_mip(texture, uv, None, "clamp", lod)
    assert bool(valid.all())
    levels = [texture.permute(0, 3, 1, 2)]
    for k in range(1, L):
        h, w = levels[-1].shape[-2:]
        levels.append(Fn.avg_pool2d(levels[-1], (2 if h > 1 else 1, 2 if w > 1 else 1)))
    per_level = torch.stack([Fn.grid_sample(t, 2.0 * uv - 1.0, mode="bilinear", padding_mode="border",
                                            align_corners=False).permute(0, 2, 3, 1) for t in levels])
    k0 = lod.floor().long()
    k1 = torch.clamp(k0 + 1, max=L - 1)
    f = (lod - k0)[..., None]
    pick = lambda k: torch.gather(per_level, 0, k[None, ..., None].expand((1, B, H, W, C)))[0]  # noqa: E731
    ref = pick(k0) * (1 - f) + pick(k1) * f
    assert float((got - ref).detach().abs().max()) <= 1e-12
    for a, b in zip(torch.autograd.grad(got, [texture, uv], g), torch.autograd.grad(ref, [texture, uv], g)):
        assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))


def test_lod_rule_examples():
    """The piecewise-linear log2: exact at powers of two, within 0.044 of 0.5 * log2(rho2), monotone; the bit-field
    form (the kernel's) and the frexp form (the statement's) agree on every value tried."""
    rng = np.random.default_rng(3)
    rho2 = np.concatenate([2.0 ** np.arange(0, 40), rng.uniform(1, 2 ** 30, 100000),
                           np.exp(rng.uniform(0, 80, 100000))]).astype(np.float32)
    m, e = np.frexp(rho2)
    a = np.float32(0.5) * ((e - 1).astype(np.float32) + (m * np.float32(2) - np.float32(1)))
    bits = rho2.view(np.uint32)
    mant = ((bits & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(np.float32)
    b = np.float32(0.5) * (((bits >> 23).astype(np.int32) - 127).astype(np.float32) + (mant - np.float32(1)))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a[:40], 0.5 * np.arange(0, 40))
    assert np.abs(a - 0.5 * np.log2(rho2.astype(np.float64))).max() < 0.044
    order = np.argsort(rho2)
    assert np.all(np.diff(a[order]) >= 0)
    # through the public entry: a uv moving exactly 4 texels per pixel in x, 1 in y, over a 64 x 64 chain
    y, x = np.meshgrid(np.arange(4.0), np.arange(4.0), indexing="ij")
    uv = np.stack([x * 4 / 64, y / 64], -1).astype(np.float32)
    lod = deferred._sample_texture_mip(torch.zeros((64, 64, 1)), torch.from_numpy(uv))[2]
    assert lod.shape == (4, 4) and bool((lod == 2.0).all())
    lod = deferred._sample_texture_mip(torch.zeros((64, 64, 1)), torch.from_numpy(uv), lod_bias=0.5)[2]
    assert bool((lod == 2.5).all())
    lod = deferred._sample_texture_mip(torch.zeros((64, 64, 1)), torch.from_numpy(uv), lod_bias=-5.0)[2]
    assert bool((lod == 0.0).all())


def test_public_surface():
    t, uv = torch.rand((8, 4, 3)), torch.rand((2, 3, 2))
    m = deferred.build_mipmaps(t)
    assert len(m) == 4 and m.dims == ((8, 4), (4, 2), (2, 1), (1, 1)) and m.packed.shape == (43, 3)
    assert m.level(1).shape == (4, 2, 3) and m.level(1).data_ptr() == m.packed[32:].data_ptr()  # (a view)
    assert len(deferred.build_mipmaps(t, levels=2)) == 2 and len(deferred.build_mipmaps(t, levels=9)) == 4
    assert deferred.sample_texture_mip(m, uv)[0].shape == (2, 3, 3)
    assert deferred.sample_texture_mip(t, uv[None])[1].shape == (1, 2, 3, 1)
    mb = deferred.build_mipmaps(torch.rand((2, 8, 4, 3)))
    assert mb.packed.shape == (2, 43, 3) and mb.level(2).shape == (2, 2, 1, 3)
    assert deferred.sample_texture_mip(mb, torch.rand((2, 6, 7, 2)))[0].shape == (2, 6, 7, 3)
    # a user's own chain
    own = deferred.Mipmaps(torch.rand((43, 3)), 8, 4)
    assert len(own) == 4 and deferred.sample_texture_mip(own, uv, lod=torch.ones((2, 3)))[0].shape == (2, 3, 3)
    assert len(deferred.Mipmaps(torch.rand((40, 3)), 8, 4, 2)) == 2
    # differentiable to the texture through the chain
    tt = t.clone().requires_grad_(True)
    deferred.sample_texture_mip(deferred.build_mipmaps(tt), uv, lod=torch.full((2, 3), 1.5))[0].sum().backward()
    assert bool((tt.grad != 0).all())
    # a constant texture is constant at every lod; unsampled pixels are exactly 0
    texels, valid = deferred.sample_texture_mip(torch.full((4, 4, 1), 7.0),
                                                torch.tensor([[[0.3, 5.0], [0.5, float("-inf")]]]), lod_bias=1.0)
    assert valid.reshape(-1).tolist() == [True, False] and texels.reshape(-1).tolist() == [7.0, 0.0]
    for bad in (dict(wrap="mirror"), dict(wrap=0)):
        with pytest.raises(ValueError, match="wrap"):
            deferred.sample_texture_mip(m, uv, **bad)
    for bad_uv in (torch.zeros((2, 3, 3)), torch.zeros((2,)), torch.zeros((1, 1, 2, 3, 2))):
        with pytest.raises(ValueError, match="uv must be"):
            deferred.sample_texture_mip(m, bad_uv)
    for bad_t in (torch.zeros((4, 5)), torch.zeros((0, 5, 3)), torch.zeros((1, 1, 4, 5, 3))):
        with pytest.raises(ValueError, match="texture must be"):
            deferred.build_mipmaps(bad_t)
    for bad_levels in (0, -1, 1.5):
        with pytest.raises(ValueError, match="levels"):
            deferred.build_mipmaps(t, levels=bad_levels)
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_texture_mip(mb, torch.zeros((3, 6, 7, 2)))
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_texture_mip(mb, uv)
    with pytest.raises(ValueError, match="mask of shape"):
        deferred.sample_texture_mip(m, uv, torch.zeros((3, 2)))
    with pytest.raises(ValueError, match="lod must be"):
        deferred.sample_texture_mip(m, uv, lod=torch.zeros((3, 2)))
    with pytest.raises(ValueError, match="lod must be"):
        deferred.sample_texture_mip(m, uv, lod=torch.zeros((2, 3), dtype=torch.int64))
    for bad_bias in (float("nan"), float("inf"), torch.tensor(0.5)):
        with pytest.raises(ValueError, match="lod_bias"):
            deferred.sample_texture_mip(m, uv, lod_bias=bad_bias)
    with pytest.raises(ValueError, match="packed must be"):
        deferred.Mipmaps(torch.rand((42, 3)), 8, 4)
    with pytest.raises(ValueError, match="levels"):
        deferred.Mipmaps(torch.rand((43, 3)), 8, 4, 5)


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dirt_mi355x.h")).read()
    assert "#define DIRT_MAX_MIP_LEVELS %d" % _lib.MAX_MIP_LEVELS in header
    assert "no gradient" in header.lower() and "no gradient" in deferred.sample_texture_mip.__doc__


def _args(fn, frames=1, Th=8, Tw=8, C=3, levels=0, B=1, H=4, W=4, wrap=0, bias=0.0, null=()):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    if fn == "dirt_texture_mip_build_fwd":
        return [p("texture"), frames, Th, Tw, C, levels, p("packed"), None], word
    if fn == "dirt_texture_mip_build_bwd":
        return [p("grad_packed"), frames, Th, Tw, C, levels, p("grad_texture"), None], word
    head = [p("packed"), frames, Th, Tw, C, levels, p("uv"), None]
    if fn == "dirt_texture_sample_mip_fwd":
        return head + [None, bias, B, H, W, wrap, p("texels"), p("valid"), p("lod"), None], word
    return head + [p("lod"), B, H, W, wrap, p("grad_texels"), p("grad_packed"), p("grad_uv"), None], word


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    big = _lib.MAX_DIM + 1
    every = ("texture", "packed", "grad_packed", "grad_texture", "uv", "texels", "valid", "lod", "grad_texels",
             "grad_uv")
    for fn in NEW_SYMBOLS[1:]:
        f = getattr(lib, fn)
        sample = "sample" in fn
        cases = [(dict(Th=0), "texture height, width"), (dict(Tw=0), "texture height, width"),
                 (dict(Th=big), "texture height, width"), (dict(Tw=big), "texture height, width"),
                 (dict(C=0), "channels"), (dict(C=_lib.MAX_CHANNELS + 1), "channels"),
                 (dict(levels=5), "levels"), (dict(Th=6, Tw=10, levels=3), "levels"), (dict(Th=5, levels=2), "levels"),
                 (dict(frames=-1), "texture_frames")]
        if sample:
            cases += [(dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=big), "height, width"),
                      (dict(frames=2), "texture_frames"), (dict(frames=0), "texture_frames"),
                      (dict(frames=2, B=3), "texture_frames"), (dict(wrap=2), "wrap"), (dict(wrap=-1), "wrap")]
        for bad, msg in cases:
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err(), (fn, bad, err())
        # nothing to do, whatever the pointers
        a, _keep = _args(fn, null=every, **(dict(B=0) if sample else dict(frames=0)))
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, Th=0, null=every)
        assert f(*a) == _lib.DIRT_EINVAL and "texture height, width" in err(), fn
    for bias in (float("nan"), float("inf")):
        a, _keep = _args("dirt_texture_sample_mip_fwd", bias=bias)
        assert lib.dirt_texture_sample_mip_fwd(*a) == _lib.DIRT_EINVAL and "lod_bias" in err()
    required = {"dirt_texture_mip_build_fwd": ("texture", "packed"),
                "dirt_texture_mip_build_bwd": ("grad_packed", "grad_texture"),
                "dirt_texture_sample_mip_fwd": ("packed", "uv", "texels", "valid", "lod"),
                "dirt_texture_sample_mip_bwd": ("packed", "uv", "lod", "grad_texels")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the backward with no gradient requested: no work and no error
    a, _keep = _args("dirt_texture_sample_mip_bwd", null=("grad_packed", "grad_uv", "packed", "grad_texels"))
    assert lib.dirt_texture_sample_mip_bwd(*a) == _lib.DIRT_OK
