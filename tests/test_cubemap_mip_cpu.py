"""dirt_amd.deferred.build_cubemap_mipmaps / sample_cubemap_mip on a CPU: the framework-op statement
`_sample_cubemap_mip_ops` against the numpy statement of record (tests/cubemap_mip_cases.py) on its whole table, the
clamped form against `_sample_cubemap_ops`, the continuity across the 12 seams and 8 corners that the seamless rule is
for, double backward, the public entries' argument checks and the two C entry points' (no GPU call is made).
"""
import ctypes

import numpy as np
import pytest
import torch

import cubemap_mip_cases as cm
import texture_mip_cases as tmc
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_texture_sample_cube_mip_fwd", "dirt_texture_sample_cube_mip_bwd")


def _t(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ratio(err, bound, tag):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    zero = bound == 0
    assert not np.any(err[zero]), tag
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize("ident", cm.CASE_IDS)
def test_ops_match_the_statement(ident):
    """float32: the chain, texels, valid and the final lod bit-equal to the numpy statement, unsampled pixels exactly
    0; the public entries take the same route on a CPU.  The gradients of the float32 ops to the cube map (through
    the chain), the directions and an explicit lod within the statement's derived bounds of its float64 vjp."""
    inp, chain, fwd, vjp = cm.case(ident)
    C = inp["cubemap"].shape[-1]
    ct = _t(inp["cubemap"]).requires_grad_(True)
    dt = _t(inp["directions"]).requires_grad_(True)
    lt = None if inp["lod"] is None else _t(inp["lod"]).requires_grad_(True)
    built = deferred.build_cubemap_mipmaps(ct)
    assert isinstance(built, deferred.CubeMipmaps) and len(built) == len(chain)
    assert np.array_equal(_bits(built.packed.detach().numpy()), _bits(cm.pack(chain))), ident
    for k, level in enumerate(chain):
        assert np.array_equal(_bits(built.level(k).detach().numpy()), _bits(level)), (ident, k)
    texels, valid, lod = deferred._sample_cubemap_mip_ops(built, dt, _t(inp["mask"]), lt, inp["lod_bias"],
                                                          inp["seamless"])
    assert valid.dtype == torch.bool and tuple(valid.shape) == fwd["valid"].shape + (1,)
    assert np.array_equal(valid.numpy()[..., 0], fwd["valid"]), ident
    assert np.array_equal(_bits(lod.numpy()), _bits(fwd["lod"])), ident
    assert np.array_equal(_bits(texels.detach().numpy()), _bits(fwd["texels"])), ident
    assert not np.any(_bits(texels.detach().numpy())[~fwd["valid"]]), ident
    pub = deferred.sample_cubemap_mip(built, dt, _t(inp["mask"]), lt, inp["lod_bias"], inp["seamless"])
    assert torch.equal(pub[0], texels) and torch.equal(pub[1], valid)
    if not fwd["valid"].any():
        return
    wanted = [ct, dt] + ([lt] if lt is not None else [])
    grads = [g.numpy() for g in torch.autograd.grad(texels, wanted, _t(inp["grad"]))]
    r_c = _ratio(np.abs(grads[0] - vjp["grad_cubemap"]), vjp["cubemap_bound"], ident)
    r_d = _ratio(np.abs(grads[1] - vjp["grad_directions"]), cm.directions_bound(vjp, C), ident)
    assert not np.any(grads[1][~fwd["valid"]]), ident
    r_l = 0.0
    if lt is not None:
        r_l = _ratio(np.abs(grads[2] - vjp["grad_lod"]), cm.lod_bound(vjp, C), ident)
        assert not np.any(grads[2][~fwd["passes"]]), ident
    print("cubemap mip ops %s: grad_cubemap %.3f, grad_directions %.3f, grad_lod %.3f of their bounds"
          % (ident, r_c, r_d, r_l))
    assert r_c <= 1.0 and r_d <= 1.0 and r_l <= 1.0, (ident, r_c, r_d, r_l)


@pytest.mark.parametrize("ident", [i for i in cm.CASE_IDS if "15x17" in i or "3x5x6" in i][:12])
def test_ops_in_float64(ident):
    """the ops in float64 against the statement evaluated in float64 on the same inputs: texels to 1e-12, the
    gradients of autograd to 1e-10 of the sums of the absolute terms"""
    inp = cm.case_input(ident)
    chain, f64, vjp = cm.statement(inp, np.float64)
    ct = _t(inp["cubemap"], torch.float64).requires_grad_(True)
    dt = _t(inp["directions"], torch.float64).requires_grad_(True)
    lt = None if inp["lod"] is None else _t(inp["lod"], torch.float64).requires_grad_(True)
    texels, valid = deferred.sample_cubemap_mip(ct, dt, _t(inp["mask"]), lt, inp["lod_bias"], inp["seamless"])
    assert np.array_equal(valid.numpy()[..., 0], f64["valid"])
    assert np.abs(texels.detach().numpy() - f64["texels"]).max() <= 1e-12
    if not f64["valid"].any():
        return
    wanted = [ct, dt] + ([lt] if lt is not None else [])
    grads = [g.numpy() for g in torch.autograd.grad(texels, wanted, _t(inp["grad"], torch.float64))]
    S = inp["cubemap"].shape[-2]
    abs_cubemap = cm.chain_vjp(vjp["S"], S)
    assert np.all(np.abs(grads[0] - vjp["grad_cubemap"]) <= 1e-10 * abs_cubemap), ident
    assert np.all(np.abs(grads[1] - vjp["grad_directions"]) <= 1e-10 * vjp["abs_directions"]), ident
    if lt is not None:
        assert np.all(np.abs(grads[2] - vjp["grad_lod"]) <= 1e-10 * vjp["abs_lod"]), ident


@pytest.mark.parametrize("ident", ["15x17-s5-c3-shared-lattice-frac", "17x33-s8-c4-perframe-random-int-mask",
                                   "17x33-s64-c3-shared-corner-frac-bg"])
def test_clamped_at_lod_zero_is_sample_cubemap(ident):
    """seamless=False with an all-zero explicit lod is `_sample_cubemap_ops`, bit for bit"""
    inp = cm.case_input(ident)
    c, d, m = _t(inp["cubemap"]), _t(inp["directions"]), _t(inp["mask"])
    got = deferred.sample_cubemap_mip(c, d, m, torch.zeros(d.shape[:-1]), 0.0, seamless=False)
    want = deferred._sample_cubemap_ops(c, d, m)
    assert torch.equal(got[1], want[1]) and bool(want[1].any())
    assert np.array_equal(_bits(got[0].numpy()), _bits(want[0].numpy()))


def test_resolve_is_an_involution_on_the_seams():
    """A folded tap lands on the texel that, folded back from there, reaches the cell next to the edge it came over:
    the two faces of a seam see each other's border texels, for every face, edge and odd or even size."""
    for T in (1, 2, 3, 8):
        for face in range(6):
            for i, j in [(-1, k) for k in range(T)] + [(T, k) for k in range(T)] + \
                        [(k, -1) for k in range(T)] + [(k, T) for k in range(T)]:
                rf, ri, rj, kind = (int(x) for x in cm.resolve(face, i, j, T))
                assert kind == 1 and rf != face and rf // 2 != face // 2
                # one of the four steps off that texel's face comes back to the cell inside (i, j)'s edge
                inside = (min(max(i, 0), T - 1), min(max(j, 0), T - 1))
                back = [tuple(int(x) for x in cm.resolve(rf, ri + di, rj + dj, T))
                        for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1))]
                assert (face,) + inside + (1,) in back, (T, face, i, j, back)
    for T in (1, 4):
        assert all(int(cm.resolve(f, i, j, T)[3]) == 2 for f in range(6) for i in (-1, T) for j in (-1, T))


def test_seamless_filtering_is_continuous():
    """A cube map sampled from a smooth function at every level, and pairs of directions a relative 1e-6 apart that
    straddle each of the 12 seams and the 8 corners.  Seamless: a pair differs by no more than the filtered function
    can change over that distance plus rounding (the value's slope is at most 2 max|t| per texel: 2e-6 * T * 2 max|t|,
    and a few units of float32 roundoff of max|t|).  Clamped: on the coarse levels the pairs jump visibly."""
    first, second, corner = cm.straddling_pairs()
    n = len(first)
    assert n == 12 * 5 + 24 and corner.sum() == 24
    S = 64
    chain = cm.smooth_chain(S)
    L = len(chain)
    scale = max(float(np.abs(c).max()) for c in chain)
    d = np.stack([first, second])[None]  # [1, 2, n, 3]
    faces = cm.sample(chain, d, None, np.zeros((1, 2, n), np.float32))["face"][0]
    assert np.all(faces[0] != faces[1])
    pairs = set(map(tuple, np.sort(faces.T[~corner], 1).tolist()))
    assert len(pairs) == 12  # every seam
    packed = deferred.CubeMipmaps(_t(cm.pack(chain)), S)
    worst_clamped = {}
    for k in range(L):
        T = S >> k
        for lod in (float(k), min(k + 0.5, L - 1.0)):
            lod_t = torch.full((1, 2, n), lod)
            want = cm.sample(chain, d, None, lod_t.numpy())
            got, _ = deferred.sample_cubemap_mip(packed, _t(d), None, lod_t)
            assert np.array_equal(_bits(got.numpy()), _bits(want["texels"]))
            jump = np.abs(want["texels"][0, 0] - want["texels"][0, 1]).max(-1)
            allowed = 2e-6 * T * 2 * scale + 16 * 2.0 ** -24 * scale
            assert np.all(jump <= allowed), (k, lod, float(jump.max()), allowed)
            clamped = cm.sample(chain, d, None, lod_t.numpy(), seamless=False)["texels"]
            worst_clamped[lod] = float(np.abs(clamped[0, 0] - clamped[0, 1]).max())
    # without the rule the coarse levels are a cube with hard edges: the 1 x 1 level jumps by the difference of two
    # faces' values, every level from 8 x 8 up by more than a hundred times what the seamless rule allows at all
    print("clamped jumps per lod:", {k: "%.3g" % v for k, v in worst_clamped.items()})
    assert worst_clamped[float(L - 1)] > 0.5
    assert all(v > 100 * (2e-6 * 8 * 2 * scale + 16 * 2.0 ** -24 * scale) for k, v in worst_clamped.items() if k >= 3)


def test_lod_gradient_at_an_integer_lod_is_the_right_derivative():
    """A roughness map initialised at 0 moves: the gradient at an integer lod is sum_c g_c * (s_k1 - s_k0), also at
    lod = 0 exactly; it is 0 at the top level, above it, below 0 and at a NaN."""
    rng = np.random.default_rng(3)
    cubemap = rng.standard_normal((6, 8, 8, 2)).astype(np.float32)
    d = rng.standard_normal((1, 1, 7, 3)).astype(np.float32)
    lod = np.array([[[0.0, 1.0, 3.0, 3.5, -0.25, np.nan, 2.0]]], np.float32)
    chain = cm.build_chain(cubemap)
    fwd = cm.sample(chain, d, None, lod)
    vjp = cm.sample_vjp(chain, np.ones((1, 1, 7, 2), np.float32), fwd)
    lt = _t(lod).requires_grad_(True)
    texels, _ = deferred.sample_cubemap_mip(_t(cubemap), _t(d), None, lt)
    g, = torch.autograd.grad(texels.sum(), [lt])
    assert np.all(vjp["grad_lod"][0, 0, [0, 1, 6]] != 0) and not np.any(vjp["grad_lod"][0, 0, 2:6])
    assert np.all(np.abs(g.numpy() - vjp["grad_lod"]) <= cm.lod_bound(vjp, 2))
    s = [cm.sample(chain, d, None, np.full((1, 1, 7), k, np.float32))["texels"].astype(np.float64) for k in (0, 1)]
    assert abs(vjp["grad_lod"][0, 0, 0] - (s[1] - s[0])[0, 0, 0].sum()) <= 1e-6


def test_double_backward_through_the_ops():
    rng = np.random.default_rng(5)
    cubemap = torch.from_numpy(rng.standard_normal((6, 4, 4, 3))).requires_grad_(True)
    d = torch.from_numpy(rng.standard_normal((3, 4, 3))).requires_grad_(True)
    lod = torch.from_numpy(rng.uniform(0.0, 2.0, (3, 4))).requires_grad_(True)
    for lod_in in (lod, None):
        texels, _ = deferred.sample_cubemap_mip(cubemap, d, None, lod_in)
        wrt = [d] + ([lod] if lod_in is not None else [])
        first = torch.autograd.grad(texels.square().sum(), wrt, create_graph=True)
        gg = torch.autograd.grad(sum(g.square().sum() for g in first), [cubemap, d] + wrt[1:])
        assert all(bool(torch.isfinite(g).all()) for g in gg) and float(gg[0].abs().sum()) > 0


def test_gradcheck_away_from_kinks():
    """directions at texel-cell interiors of the levels they read on random faces, edges included (folded taps), and
    fractional lods: autograd against central differences in float64, to the cube map, the directions and the lod"""
    rng = np.random.default_rng(6)
    S, shape = 4, (2, 3, 4)
    u = (rng.integers(0, S, shape) + rng.uniform(0.15, 0.35, shape)) / S  # (inside a cell at T = 4, 2 and 1)
    v = (rng.integers(0, S, shape) + rng.uniform(0.15, 0.35, shape)) / S
    import cubemap_cases as cc
    d = cc.on_face(rng.integers(0, 6, shape), u, v) * rng.uniform(0.5, 2.0, shape)[..., None]
    cubemap = torch.from_numpy(rng.standard_normal((2, 6, S, S, 2))).requires_grad_(True)
    d = torch.from_numpy(d).requires_grad_(True)
    lod = torch.from_numpy(rng.uniform(0.1, 0.9, shape) + rng.integers(0, 2, shape)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda c, x, l: deferred.sample_cubemap_mip(c, x, None, l)[0], (cubemap, d, lod),
                                    eps=1e-6, atol=1e-7)


def test_public_surface():
    c, d = torch.zeros((6, 4, 4, 3)), torch.ones((2, 3, 3))
    chain = deferred.build_cubemap_mipmaps(c)
    assert len(chain) == 3 and chain.packed.shape == (6, 21, 3) and chain.dims == ((4, 4), (2, 2), (1, 1))
    assert chain.offsets == (0, 16, 20) and chain.level(1).shape == (6, 2, 2, 3)
    assert len(deferred.build_cubemap_mipmaps(torch.zeros((6, 64, 64, 1)))) == 7
    assert len(deferred.build_cubemap_mipmaps(torch.zeros((6, 5, 5, 1)))) == 1
    assert len(deferred.build_cubemap_mipmaps(torch.zeros((6, 64, 64, 1)), levels=3)) == 3
    per_frame = deferred.build_cubemap_mipmaps(torch.zeros((2, 6, 4, 4, 5)))
    assert per_frame.packed.shape == (2, 6, 21, 5) and per_frame.level(2).shape == (2, 6, 1, 1, 5)
    assert deferred.sample_cubemap_mip(c, d)[0].shape == (2, 3, 3)
    assert deferred.sample_cubemap_mip(chain, d[None])[1].shape == (1, 2, 3, 1)
    assert deferred.sample_cubemap_mip(per_frame, torch.ones((2, 6, 7, 3)))[0].shape == (2, 6, 7, 5)
    wrapped = deferred.CubeMipmaps(torch.zeros((6, 21, 3)), 4)
    assert len(wrapped) == 3 and deferred.sample_cubemap_mip(wrapped, d, lod=torch.ones((2, 3)))[0].shape == (2, 3, 3)
    # a 1 x 1 level is the mean of the three faces at a corner, whatever the direction's length
    ramp = torch.arange(6.0).reshape(6, 1, 1, 1)
    out, _ = deferred.sample_cubemap_mip(ramp, torch.tensor([[[3.0, 3.0, 3.0]]]))
    assert abs(out.item() - 2.0) < 1e-6  # faces +x, +y, +z hold 0, 2, 4
    for bad_d in (torch.zeros((2, 3, 2)), torch.zeros((3,))):
        with pytest.raises(ValueError, match="directions must be"):
            deferred.sample_cubemap_mip(c, bad_d)
    for bad_c in (torch.zeros((5, 4, 4, 3)), torch.zeros((4, 4, 3)), torch.zeros((6, 0, 0, 3))):
        with pytest.raises(ValueError, match="cubemap must be"):
            deferred.build_cubemap_mipmaps(bad_c)
    with pytest.raises(ValueError, match="square"):
        deferred.build_cubemap_mipmaps(torch.zeros((6, 4, 2, 3)))
    for levels in (0, 1.5, -1):
        with pytest.raises(ValueError, match="levels"):
            deferred.build_cubemap_mipmaps(c, levels=levels)
    with pytest.raises(ValueError, match="packed must be"):
        deferred.CubeMipmaps(torch.zeros((6, 20, 3)), 4)
    with pytest.raises(ValueError, match="packed must be"):
        deferred.CubeMipmaps(torch.zeros((5, 21, 3)), 4)
    with pytest.raises(ValueError, match="levels = 4"):
        deferred.CubeMipmaps(torch.zeros((6, 21, 3)), 4, levels=4)
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_cubemap_mip(per_frame, torch.ones((3, 6, 7, 3)))
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_cubemap_mip(per_frame, d)
    with pytest.raises(ValueError, match="mask of shape"):
        deferred.sample_cubemap_mip(c, d, torch.zeros((3, 2)))
    with pytest.raises(ValueError, match="lod must be"):
        deferred.sample_cubemap_mip(c, d, lod=torch.zeros((3, 2)))
    with pytest.raises(ValueError, match="lod must be"):
        deferred.sample_cubemap_mip(c, d, lod=torch.zeros((2, 3), dtype=torch.int64))
    for bias in (float("nan"), float("inf"), torch.zeros(())):
        with pytest.raises(ValueError, match="lod_bias"):
            deferred.sample_cubemap_mip(c, d, lod_bias=bias)


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only: no signature or workspace layout changed


def _args(fn, frames=1, S=4, C=3, levels=0, B=1, H=4, W=4, seamless=1, bias=0.0, null=()):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    head = [p("packed"), frames, S, C, levels, p("directions"), None, p("lod_in"), bias]
    if fn == "dirt_texture_sample_cube_mip_fwd":
        return head + [B, H, W, seamless, p("texels"), p("valid"), p("lod"), None], word
    return head + [p("lod"), B, H, W, seamless, p("grad_texels"), p("grad_packed"), p("grad_directions"),
                   p("grad_lod"), None], word


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    big = _lib.MAX_DIM + 1
    everything = ("packed", "directions", "lod_in", "texels", "valid", "lod", "grad_texels", "grad_packed",
                  "grad_directions")
    for fn in NEW_SYMBOLS:
        f = getattr(lib, fn)
        for bad, msg in ((dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=big), "height, width"),
                         (dict(S=0), "faces' size"), (dict(S=big), "faces' size"),
                         (dict(C=0), "channels"), (dict(C=_lib.MAX_CHANNELS + 1), "channels"),
                         (dict(frames=2), "cubemap_frames"), (dict(frames=0), "cubemap_frames"),
                         (dict(levels=4), "levels = 4"), (dict(S=5, levels=2), "levels = 2"),
                         (dict(seamless=2), "seamless"), (dict(seamless=-1), "seamless"),
                         (dict(bias=float("nan")), "lod_bias"), (dict(bias=float("inf")), "lod_bias")):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err() and "texture_sample_cube" in err(), (fn, bad, err())
        a, _keep = _args(fn, B=0, null=everything + ("grad_lod",))
        assert f(*a) == _lib.DIRT_OK, fn
        a, _keep = _args(fn, S=0, null=("packed", "directions"))
        assert f(*a) == _lib.DIRT_EINVAL and "faces' size" in err(), fn
    required = {"dirt_texture_sample_cube_mip_fwd": ("packed", "directions", "texels", "valid", "lod"),
                "dirt_texture_sample_cube_mip_bwd": ("packed", "directions", "lod", "grad_texels")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # grad_lod is the gradient of lod_in: without one it is an error; with no gradient requested, no work, no error
    a, _keep = _args("dirt_texture_sample_cube_mip_bwd", null=("lod_in",))
    assert lib.dirt_texture_sample_cube_mip_bwd(*a) == _lib.DIRT_EINVAL and "grad_lod needs" in err()
    a, _keep = _args("dirt_texture_sample_cube_mip_bwd",
                     null=("grad_packed", "grad_directions", "grad_lod", "packed", "grad_texels"))
    assert lib.dirt_texture_sample_cube_mip_bwd(*a) == _lib.DIRT_OK


def test_layout_is_the_texture_chains():
    """the packed chain of a face is texture_mip_cases' layout of an S x S texture, for every size of the table"""
    for S in cm.SIZES + [6, 12]:
        dims, offsets, n = tmc.layout(S, S)
        chain = deferred.build_cubemap_mipmaps(torch.zeros((6, S, S, 1)))
        assert chain.dims == tuple(dims) and chain.offsets == tuple(offsets) and chain.packed.shape == (6, n, 1)
