"""dirt_amd.deferred.sample_cubemap on a CPU: the framework-op statement `_sample_cubemap_ops` against the numpy
statement of record (tests/cubemap_cases.py) on its whole table, the scale invariance of the direction gradient, the
lattice's face list, double backward, the public entry's argument checks and the two C entry points' (no GPU call is
made).
"""
import ctypes

import numpy as np
import pytest
import torch

import cubemap_cases as cc
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_texture_sample_cube_fwd", "dirt_texture_sample_cube_bwd")


def _t(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("ident", cc.CASE_IDS)
def test_ops_match_the_statement(ident):
    """float32: valid and face equal, texels within 5 * 2^-24 * max|texel| (four roundings on any path from a texel
    to the output, whatever the framework's kernels contract), unsampled pixels exactly 0.  float64 (the statement
    evaluated in float64 on the same inputs): texels to 1e-12, both gradients of autograd to 1e-10 of the sum of the
    absolute terms of each element, and |d . grad_d| <= 1e-9 |d| |grad_d| (the lookup is scale-invariant)."""
    (cubemap, d, mask, grad), fwd, _ = cc.case(ident)
    texels, valid = deferred._sample_cubemap_ops(_t(cubemap), _t(d), _t(mask))
    assert valid.dtype == torch.bool and tuple(valid.shape) == d.shape[:-1] + (1,)
    assert np.array_equal(valid.numpy()[..., 0], fwd["valid"]), ident
    face = deferred._cube_coordinates(_t(d), valid[..., 0])[0].numpy()
    assert np.array_equal(face[fwd["valid"]], fwd["face"][fwd["valid"]]), ident
    assert np.abs(texels.numpy() - fwd["texels"]).max() <= 5 * 2.0 ** -24 * np.abs(cubemap).max(), ident
    assert not np.any(texels.numpy().view(np.uint32)[~fwd["valid"]]), ident
    # the public entry takes the same route on a CPU
    pub = deferred.sample_cubemap(_t(cubemap), _t(d), _t(mask))
    assert torch.equal(pub[0], texels) and torch.equal(pub[1], valid)

    f64 = cc.sample(cubemap, d, mask, np.float64)
    vjp = cc.sample_vjp(cubemap, grad, f64)
    assert np.array_equal(f64["valid"], fwd["valid"])
    ct, dt = _t(cubemap, torch.float64).requires_grad_(True), _t(d, torch.float64).requires_grad_(True)
    texels, valid = deferred._sample_cubemap_ops(ct, dt, _t(mask))
    assert not valid.requires_grad
    assert np.array_equal(valid.numpy()[..., 0], f64["valid"])
    assert np.abs(texels.detach().numpy() - f64["texels"]).max() <= 1e-12
    if not fwd["valid"].any():
        return
    gc_, gd = (g.numpy() for g in torch.autograd.grad(texels, [ct, dt], _t(grad, torch.float64)))
    assert np.all(np.isfinite(gc_)) and np.all(np.isfinite(gd)), ident
    assert np.all(np.abs(gc_ - vjp["grad_cubemap"]) <= 1e-10 * vjp["S"]), ident
    assert np.all(np.abs(gd - vjp["grad_directions"]) <= 1e-10 * vjp["abs_directions"]), ident
    assert not np.any(gd[~fwd["valid"]])
    d64 = np.where(fwd["valid"][..., None], d.astype(np.float64), 0.0)
    dot = np.abs((d64 * gd).sum(-1))
    assert np.all(dot <= 1e-9 * np.linalg.norm(d64, axis=-1) * np.linalg.norm(gd, axis=-1)), ident


def test_lattice_faces():
    """the 26 nonzero points of {-1, 0, 1}^3 and their -0.0 variants: every tie of the major-axis rule (x before y
    before z), every face, against the list worked out by hand in cubemap_cases.LATTICE_FACES"""
    pts, n = cc._lattice_points()
    assert n == 26 and len(pts) == 26 + 18 and np.signbit(pts[n:][pts[n:] == 0]).all()
    shape = (1, 1, len(pts))
    want = cc.lattice_faces(shape)
    assert sorted(set(want.reshape(-1).tolist())) == list(range(6))
    for dtype in (np.float32, np.float64):
        d = pts.reshape(shape + (3,)).astype(dtype)
        fwd = cc.sample(np.zeros((6, 2, 2, 1), dtype), d, None, dtype)
        assert fwd["valid"].all() and np.array_equal(fwd["face"], want)
        face = deferred._cube_coordinates(_t(d), torch.ones(shape, dtype=torch.bool))[0]
        assert np.array_equal(face.numpy(), want)
    # each face returns its own texel: a cube map whose face k holds k + 1
    cubemap = torch.arange(1.0, 7.0).reshape(6, 1, 1, 1)
    texels, _ = deferred.sample_cubemap(cubemap, _t(pts.reshape(shape + (3,)).astype(np.float32)))
    assert np.array_equal(texels.numpy()[..., 0], want + 1.0)


def test_public_surface():
    assert callable(deferred.sample_cubemap)
    c, d = torch.zeros((6, 4, 4, 3)), torch.ones((2, 3, 3))
    assert deferred.sample_cubemap(c, d)[0].shape == (2, 3, 3)
    assert deferred.sample_cubemap(c, d[None])[1].shape == (1, 2, 3, 1)
    assert deferred.sample_cubemap(torch.zeros((2, 6, 4, 4, 5)), torch.ones((2, 6, 7, 3)))[0].shape == (2, 6, 7, 5)
    # the centre of texel (1, 0) of the +y face of a 2 x 2 ramp: sc = x = -0.5, tc = z = 0.5 -> u = 0.25, v = 0.75
    ramp = torch.arange(24.0).reshape(6, 2, 2, 1)
    assert deferred.sample_cubemap(ramp, torch.tensor([[[-1.0, 2.0, 1.0]]]))[0].item() == 10.0
    # -inf, NaN and the zero vector are unsampled, with or without a mask that is set there
    bad = torch.tensor([[[float("-inf"), 0, 0], [0, float("nan"), 1], [0, 0, 0], [-0.0, 0, -0.0], [0, 0, 3.0]]])
    for mask in (None, torch.ones((1, 5))):
        texels, valid = deferred.sample_cubemap(ramp, bad, mask)
        assert valid.reshape(-1).tolist() == [False] * 4 + [True]
        assert texels.reshape(-1).tolist() == [0.0] * 4 + [17.5]
    texels, valid = deferred.sample_cubemap(ramp, bad, torch.zeros((1, 5)))
    assert not bool(valid.any()) and not bool(texels.any())
    for bad_d in (torch.zeros((2, 3, 2)), torch.zeros((3,)), torch.zeros((1, 1, 2, 3, 3))):
        with pytest.raises(ValueError, match="directions must be"):
            deferred.sample_cubemap(c, bad_d)
    for bad_c in (torch.zeros((5, 4, 4, 3)), torch.zeros((4, 4, 3)), torch.zeros((2, 7, 4, 4, 3)),
                  torch.zeros((1, 2, 6, 4, 4, 3))):
        with pytest.raises(ValueError, match="cubemap must be"):
            deferred.sample_cubemap(bad_c, d)
    for bad_c in (torch.zeros((6, 4, 5, 3)), torch.zeros((2, 6, 5, 4, 3)), torch.zeros((6, 0, 0, 3)),
                  torch.zeros((6, 4, 4, 0))):
        with pytest.raises(ValueError, match="square"):
            deferred.sample_cubemap(bad_c, torch.ones((2, 2, 3, 3)))
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_cubemap(torch.zeros((3, 6, 4, 4, 3)), torch.ones((2, 6, 7, 3)))
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_cubemap(torch.zeros((1, 6, 4, 4, 3)), d)
    with pytest.raises(ValueError, match="mask of shape"):
        deferred.sample_cubemap(c, d, torch.zeros((3, 2)))


def test_mask_forms():
    """bool, integer and float masks, batched and unbatched, select the same pixels"""
    (cubemap, d, _, _), _, _ = cc.case("15x17-s5-c3-shared-lattice")
    mask = np.random.default_rng(4).random(d.shape[:-1]) < 0.6
    want = cc.sample(cubemap, d, mask.astype(np.uint8))
    for m in (_t(mask), _t(mask.astype(np.int64)) * 3, _t(mask.astype(np.float32)), mask.astype(np.uint8)):
        texels, valid = deferred.sample_cubemap(_t(cubemap), _t(d), m)
        assert np.array_equal(valid.numpy()[..., 0], want["valid"])
        assert np.abs(texels.numpy() - want["texels"]).max() <= 5 * 2.0 ** -24 * np.abs(cubemap).max()
    texels, valid = deferred.sample_cubemap(_t(cubemap), _t(d[0]), _t(mask[0]))
    assert texels.shape == (15, 17, 3) and np.array_equal(valid.numpy()[..., 0], want["valid"][0])


def test_double_backward_through_the_ops():
    rng = np.random.default_rng(5)
    cubemap = torch.from_numpy(rng.standard_normal((6, 5, 5, 3))).requires_grad_(True)
    d = torch.from_numpy(rng.standard_normal((3, 4, 3))).requires_grad_(True)
    texels, _ = deferred._sample_cubemap_ops(cubemap, d)
    gd, = torch.autograd.grad(texels.square().sum(), [d], create_graph=True)
    gg_c, gg_d = torch.autograd.grad(gd.square().sum(), [cubemap, d])
    assert bool(torch.isfinite(gg_c).all()) and bool(torch.isfinite(gg_d).all()) and float(gg_c.abs().sum()) > 0


def test_gradcheck_away_from_kinks():
    """directions at texel-cell interiors of random faces (x = j + 0.2 .. j + 0.8), lengths varying"""
    rng = np.random.default_rng(6)
    S, shape = 5, (2, 3, 4)
    u = (rng.integers(0, S - 1, shape) + rng.uniform(0.7, 1.3, shape)) / S
    v = (rng.integers(0, S - 1, shape) + rng.uniform(0.7, 1.3, shape)) / S
    d = cc.on_face(rng.integers(0, 6, shape), u, v) * rng.uniform(0.5, 2.0, shape)[..., None]
    cubemap = torch.from_numpy(rng.standard_normal((2, 6, S, S, 2))).requires_grad_(True)
    d = torch.from_numpy(d).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda c, x: deferred._sample_cubemap_ops(c, x)[0], (cubemap, d), eps=1e-6,
                                    atol=1e-7)


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only: no signature or workspace layout changed


def _args(fn, frames=1, S=4, C=3, B=1, H=4, W=4, null=()):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    head = [p("cubemap"), frames, S, C, p("directions"), None, B, H, W]
    if fn == "dirt_texture_sample_cube_fwd":
        return head + [p("texels"), p("valid"), None], word
    return head + [p("grad_texels"), p("grad_cubemap"), p("grad_directions"), None], word


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    big = _lib.MAX_DIM + 1
    assert big == 8193
    everything = ("cubemap", "directions", "texels", "valid", "grad_texels", "grad_cubemap", "grad_directions")
    for fn in NEW_SYMBOLS:
        f = getattr(lib, fn)
        for bad, msg in ((dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=0), "height, width"),
                         (dict(H=big), "height, width"), (dict(W=big), "height, width"),
                         (dict(S=0), "faces' size"), (dict(S=-3), "faces' size"), (dict(S=big), "faces' size"),
                         (dict(C=0), "channels"), (dict(C=_lib.MAX_CHANNELS + 1), "channels"),
                         (dict(frames=2), "cubemap_frames"), (dict(frames=0), "cubemap_frames"),
                         (dict(frames=2, B=3), "cubemap_frames")):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err() and "texture_sample_cube" in err(), (fn, bad, err())
        # B == 0: nothing to do, whatever the pointers
        a, _keep = _args(fn, B=0, null=everything)
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, S=0, null=("cubemap", "directions"))
        assert f(*a) == _lib.DIRT_EINVAL and "faces' size" in err(), fn
    required = {"dirt_texture_sample_cube_fwd": ("cubemap", "directions", "texels", "valid"),
                "dirt_texture_sample_cube_bwd": ("cubemap", "directions", "grad_texels")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the backward with no gradient requested: no work and no error
    a, _keep = _args("dirt_texture_sample_cube_bwd", null=("grad_cubemap", "grad_directions", "cubemap", "grad_texels"))
    assert lib.dirt_texture_sample_cube_bwd(*a) == _lib.DIRT_OK
