"""dirt_amd.deferred.sample_texture on a CPU: the framework-op statement `_sample_texture_ops` against the numpy
statement of record (tests/texture_cases.py) on its whole table, torch.autograd.gradcheck, grid_sample as a witness
of the clamp rule, double backward, the public entry's argument checks and the two C entry points' (no GPU call is
made).
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import texture_cases as tc
from dirt_amd import _lib, deferred

NEW_SYMBOLS = ("dirt_texture_sample_fwd", "dirt_texture_sample_bwd")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _t(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("ident", tc.CASE_IDS)
def test_ops_match_the_statement(ident):
    """float32: texels and valid bit for bit, unsampled pixels exactly 0.  float64 (the statement evaluated in float64
    on the same inputs): gradients within 1e-12 of the statement's scale."""
    (texture, uv, mask, wrap, grad), fwd, _ = tc.case(ident)
    texels, valid = deferred._sample_texture_ops(_t(texture), _t(uv), _t(mask), wrap)
    assert valid.dtype == torch.bool and tuple(valid.shape) == uv.shape[:-1] + (1,)
    assert np.array_equal(valid.numpy()[..., 0], fwd["valid"]), ident
    assert np.array_equal(_bits(texels.numpy()), _bits(fwd["texels"])), ident
    assert not np.any(_bits(texels.numpy())[~fwd["valid"]]), ident
    # the public entry takes the same route on a CPU
    pub = deferred.sample_texture(_t(texture), _t(uv), _t(mask), wrap)
    assert np.array_equal(_bits(pub[0].numpy()), _bits(fwd["texels"])) and torch.equal(pub[1], valid)

    f64 = tc.sample(texture, uv, mask, wrap, np.float64)
    vjp = tc.sample_vjp(texture, grad, f64)
    tt, ut = _t(texture, torch.float64).requires_grad_(True), _t(uv, torch.float64).requires_grad_(True)
    texels, valid = deferred._sample_texture_ops(tt, ut, _t(mask), wrap)
    assert not valid.requires_grad
    assert np.abs(texels.detach().numpy() - f64["texels"]).max() <= 1e-12
    if not fwd["valid"].any():
        return
    gt, gu = torch.autograd.grad(texels, [tt, ut], _t(grad, torch.float64))
    for name, got in (("grad_texture", gt), ("grad_uv", gu)):
        got = got.numpy()
        assert np.all(np.isfinite(got)), (ident, name)
        assert np.abs(got - vjp[name]).max() <= 1e-12 * max(1.0, np.abs(vjp[name]).max()), (ident, name)
    assert not np.any(gu.numpy()[~fwd["valid"]])


def _smooth_case(Th, Tw, C, B, per_frame, seed):
    """uv well inside texel cells and inside (0, 1): away from every kink of the rule"""
    rng = np.random.default_rng(seed)
    H, W = 3, 4
    j = rng.integers(0, Tw, (B, H, W)) + rng.uniform(0.7, 1.3, (B, H, W))  # x = j + 0.2 .. j + 0.8
    i = rng.integers(0, Th, (B, H, W)) + rng.uniform(0.7, 1.3, (B, H, W))
    uv = np.stack([np.clip(j / Tw, 0.02, 0.98), np.clip(i / Th, 0.02, 0.98)], -1)
    texture = rng.standard_normal(((B,) if per_frame else ()) + (Th, Tw, C))
    return torch.from_numpy(texture).requires_grad_(True), torch.from_numpy(uv).requires_grad_(True)


@pytest.mark.parametrize("wrap,per_frame", [("clamp", False), ("repeat", True)])
def test_gradcheck_away_from_kinks(wrap, per_frame):
    texture, uv = _smooth_case(5, 7, 2, 2, per_frame, 3)
    assert torch.autograd.gradcheck(lambda t, u: deferred._sample_texture_ops(t, u, None, wrap)[0], (texture, uv),
                                    eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("tex", tc.TEXTURES)
def test_clamp_rule_is_grid_sample_border(tex):
    """float64, uv in [-0.2, 1.2]: values, d/dtexture and d/duv equal grid_sample(bilinear, border,
    align_corners=False) on 2 * uv - 1."""
    rng = np.random.default_rng(tex[0] * 100 + tex[1])
    B, H, W, C = 2, 9, 11, 3
    texture = torch.from_numpy(rng.standard_normal((B,) + tex + (C,))).requires_grad_(True)
    uv = torch.from_numpy(rng.uniform(-0.2, 1.2, (B, H, W, 2))).requires_grad_(True)
    g = torch.from_numpy(rng.standard_normal((B, H, W, C)))
    got, valid = deferred._sample_texture_ops(texture, uv, None, "clamp")
    assert bool(valid.all())
    ref = Fn.grid_sample(texture.permute(0, 3, 1, 2), 2.0 * uv - 1.0, mode="bilinear", padding_mode="border",
                         align_corners=False).permute(0, 2, 3, 1)
    assert float((got - ref).detach().abs().max()) <= 1e-12
    for a, b in zip(torch.autograd.grad(got, [texture, uv], g), torch.autograd.grad(ref, [texture, uv], g)):
        assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("wrap", tc.WRAPS)
def test_double_backward_through_the_ops(wrap):
    texture, uv = _smooth_case(5, 7, 3, 1, False, 5)
    texels, _ = deferred._sample_texture_ops(texture, uv, None, wrap)
    gu, = torch.autograd.grad(texels.square().sum(), [uv], create_graph=True)
    gg_t, gg_u = torch.autograd.grad(gu.square().sum(), [texture, uv])
    assert bool(torch.isfinite(gg_t).all()) and bool(torch.isfinite(gg_u).all()) and float(gg_t.abs().sum()) > 0


def test_public_surface():
    assert callable(deferred.sample_texture)
    t, uv = torch.zeros((4, 5, 3)), torch.zeros((2, 3, 2))
    assert deferred.sample_texture(t, uv)[0].shape == (2, 3, 3)
    assert deferred.sample_texture(t, uv[None])[1].shape == (1, 2, 3, 1)
    assert deferred.sample_texture(torch.zeros((2, 4, 5, 3)), torch.zeros((2, 6, 7, 2)))[0].shape == (2, 6, 7, 3)
    # one texel: a constant; the centre of texel (1, 2) of a 2 x 4 ramp: its value
    assert deferred.sample_texture(torch.full((1, 1, 1), 7.0), torch.tensor([[[0.3, 5.0]]]))[0].item() == 7.0
    ramp = torch.arange(8.0).reshape(2, 4, 1)
    assert deferred.sample_texture(ramp, torch.tensor([[[2.5 / 4, 1.5 / 2]]]))[0].item() == 6.0
    texels, valid = deferred.sample_texture(ramp, torch.tensor([[[0.5, float("-inf")], [0.5, 0.5]]]))
    assert valid.reshape(-1).tolist() == [False, True] and texels.reshape(-1).tolist() == [0.0, 3.5]
    for bad in (dict(wrap="mirror"), dict(wrap=0)):
        with pytest.raises(ValueError, match="wrap"):
            deferred.sample_texture(t, uv, **bad)
    for bad_uv in (torch.zeros((2, 3, 3)), torch.zeros((2,)), torch.zeros((1, 1, 2, 3, 2))):
        with pytest.raises(ValueError, match="uv must be"):
            deferred.sample_texture(t, bad_uv)
    for bad_t in (torch.zeros((4, 5)), torch.zeros((0, 5, 3)), torch.zeros((1, 1, 4, 5, 3))):
        with pytest.raises(ValueError, match="texture must be"):
            deferred.sample_texture(bad_t, uv)
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_texture(torch.zeros((3, 4, 5, 3)), torch.zeros((2, 6, 7, 2)))
    with pytest.raises(ValueError, match="per-frame"):
        deferred.sample_texture(torch.zeros((1, 4, 5, 3)), uv)
    with pytest.raises(ValueError, match="mask of shape"):
        deferred.sample_texture(t, uv, torch.zeros((3, 2)))


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only: no signature or workspace layout changed
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dirt_mi355x.h")).read()
    assert "#define DIRT_TEXTURE_CLAMP %d" % _lib.TEXTURE_CLAMP in header
    assert "#define DIRT_TEXTURE_REPEAT %d" % _lib.TEXTURE_REPEAT in header


def _args(fn, frames=1, Th=4, Tw=4, C=3, B=1, H=4, W=4, wrap=0, null=()):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    head = [p("texture"), frames, Th, Tw, C, p("uv"), None, B, H, W, wrap]
    if fn == "dirt_texture_sample_fwd":
        return head + [p("texels"), p("valid"), None], word
    return head + [p("grad_texels"), p("grad_texture"), p("grad_uv"), None], word


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    big = _lib.MAX_DIM + 1
    for fn in NEW_SYMBOLS:
        f = getattr(lib, fn)
        for bad, msg in ((dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=0), "height, width"),
                         (dict(H=big), "height, width"), (dict(W=big), "height, width"),
                         (dict(Th=0), "texture height, width"), (dict(Tw=0), "texture height, width"),
                         (dict(Th=big), "texture height, width"), (dict(Tw=big), "texture height, width"),
                         (dict(C=0), "channels"), (dict(C=_lib.MAX_CHANNELS + 1), "channels"),
                         (dict(frames=2), "texture_frames"), (dict(frames=0), "texture_frames"),
                         (dict(frames=2, B=3), "texture_frames"), (dict(wrap=2), "wrap"), (dict(wrap=-1), "wrap")):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err(), (fn, bad, err())
        # B == 0: nothing to do, whatever the pointers
        a, _keep = _args(fn, B=0, null=("texture", "uv", "texels", "valid", "grad_texels", "grad_texture", "grad_uv"))
        assert f(*a) == _lib.DIRT_OK, fn
        # a bad size is reported before a null pointer is
        a, _keep = _args(fn, Th=0, null=("texture", "uv"))
        assert f(*a) == _lib.DIRT_EINVAL and "texture height, width" in err(), fn
    required = {"dirt_texture_sample_fwd": ("texture", "uv", "texels", "valid"),
                "dirt_texture_sample_bwd": ("texture", "uv", "grad_texels")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the backward with no gradient requested: no work and no error
    a, _keep = _args("dirt_texture_sample_bwd", null=("grad_texture", "grad_uv", "texture", "grad_texels"))
    assert lib.dirt_texture_sample_bwd(*a) == _lib.DIRT_OK
