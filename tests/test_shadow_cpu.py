"""deferred.sample_shadow on a CPU: the numpy statement of record (tests/shadow_cases.py) covers what its table claims;
its hand-derived vector-Jacobian products against central differences in float64; the framework-op statement
`_sample_shadow_ops` against it in float64 (1e-12 of scale); the convention against geometry (a floor under a
rectangular occluder, the depth map rendered by the CPU oracle under an orthographic and a perspective light); the
argument checks of the Python op and of the C ABI, which return before any GPU call.
"""
import ctypes

import numpy as np
import pytest
import torch

import deferred_pipeline as dp
import shadow_cases as sc
from dirt_amd import _lib, deferred, matrices

NEW_SYMBOLS = ("dirt_shadow_sample_workspace", "dirt_shadow_sample_fwd", "dirt_shadow_sample_bwd")


# ---- the statement alone

@pytest.mark.parametrize("ident", sc.RANDOM_CASE_IDS)
def test_random_cases_cover_their_classes(ident):
    shares = sc.classes(sc.case_forward(ident))
    for name in sc.claimed_classes(ident):
        assert shares[name] >= 0.05, (ident, name, shares)


def test_table_covers_what_it_claims():
    rows = sc.TABLE
    assert {r[1] for r in rows} == set(sc.FRAMES) and {r[2] for r in rows} == set(sc.MAPS)
    for B in (2, 3):
        forms = {(r[3], r[4]) for r in rows if sc.FRAMES[r[1]][0] == B}
        assert forms == {(False, False), (False, True), (True, False), (True, True)}, B
    assert {(r[5], r[6], r[7]) for r in rows} >= {(light, soft, biased) for light in ("ortho", "persp")
                                                   for soft in (False, True) for biased in (False, True)}
    assert {r[9] for r in rows} == {None, "bg", "mask"}
    tiles = dict.fromkeys(sc.DISPOSITIONS, 0)
    behind = infinite = 0
    for r in rows:
        inputs, fwd = sc.case_input(r[0]), sc.case_forward(r[0])
        for k, n in sc.dispositions(fwd).items():
            tiles[k] += n
        infinite += int(np.isposinf(inputs[0]).any() and np.isneginf(inputs[0]).any())
        if r[5] == "persp":
            pos, M = inputs[1].astype(np.float64), np.asarray(inputs[2], np.float64)
            M = (M[None] if M.ndim == 2 else M)[:, None, None]
            with np.errstate(invalid="ignore"):
                cw = (pos * M[..., :3, 3]).sum(-1) + M[..., 3, 3]
                behind += int((fwd["valid"] & (cw <= 0)).sum())
    assert all(tiles[k] > 0 for k in sc.DISPOSITIONS), tiles
    assert behind > 100 and infinite > 20
    # more than 256 tiles in one frame: the second kernel's strided loop
    B, H, W = sc.FRAMES["264x256"]
    assert -(-H // sc.TILE) * -(-W // sc.TILE) > 256
    for kind, want in (("magnify16", "patch"), ("scatter", "direct")):
        disp = sc.dispositions(sc.exact_scatter_case(kind)[1])
        assert disp[want] == sum(disp.values()) > 0, (kind, disp)


def _smooth_pixels(fwd, margin=1e-3):
    """inside pixels at which the visibility is differentiable with a margin: every tap's t at least `margin` from
    the ramp's two ends (softness 0: every finite texel at least `margin` from zc), the weights from 0 and 1"""
    ok = fwd["inside"].copy()
    for k in ("a", "b"):
        ok &= (fwd[k] > margin) & (fwd[k] < 1 - margin)
    return ok


@pytest.mark.parametrize("light,softness", [("ortho", 0.3), ("persp", 0.3), ("ortho", 0.0), ("persp", 0.0)])
def test_statement_vjp_against_central_differences(light, softness):
    """L = sum(g * visibility) over the pixels where the rule is smooth; its derivative to every depth texel, every
    matrix entry and (a pixel depends on its own position only) every position channel, by central differences with
    step 1e-6 in float64, against sample_vjp within 1e-6 of the gradient's scale."""
    rng = np.random.default_rng(5)
    shape, (Sh, Sw), h = (2, 15, 17), (5, 7), 1e-6
    M = sc.light_matrix(light, rng).astype(np.float64)
    pos = sc._positions_random(shape, light, Sh, Sw, rng)
    cz = sc.sample(np.zeros((Sh, Sw, 1)), pos, M, dtype=np.float64)
    zin = cz["cz"][cz["inside"]]
    depth = rng.uniform(zin.min(), zin.max(), (Sh, Sw, 1))
    depth[1, 2], depth[3, 5] = np.inf, -np.inf
    bias = 0.03
    fwd = sc.sample(depth, pos, M, bias, softness, dtype=np.float64)
    ok = _smooth_pixels(fwd)
    with np.errstate(invalid="ignore"):
        if softness > 0:
            t = fwd["t"]
            ok &= ((np.abs(t) > 1e-3) & (np.abs(t - 1) > 1e-3)).all(-1)
        else:
            d = np.stack([depth[..., 0][fwd["i0"], fwd["j0"]], depth[..., 0][fwd["i0"], fwd["j1"]],
                          depth[..., 0][fwd["i1"], fwd["j0"]], depth[..., 0][fwd["i1"], fwd["j1"]]], -1)
            ok &= (np.abs(d - (fwd["cz"] - bias)[..., None]) > 1e-3).all(-1)
    assert ok.sum() > 50
    g = np.where(ok, rng.standard_normal(shape), 0.0)
    vjp = sc.sample_vjp(depth, pos, M, g, fwd)

    def loss(depth_, pos_, M_, per_pixel=False):
        vis = sc.sample(depth_, pos_, M_, bias, softness, dtype=np.float64)["visibility"]
        return g * vis if per_pixel else float((g * vis).sum())

    scale = lambda x: max(1.0, float(np.abs(x).max()))  # noqa: E731
    finite = np.isfinite(depth)
    num = np.zeros(depth.shape)
    for idx in zip(*np.nonzero(finite)):
        e = np.zeros(depth.shape)
        e[idx] = h
        num[idx] = (loss(np.where(finite, depth + e, depth), pos, M) - loss(np.where(finite, depth - e, depth), pos, M)) \
            / (2 * h)
    assert np.abs(num - vjp["grad_depth"]).max() <= 1e-6 * scale(vjp["grad_depth"])
    assert not np.any(vjp["grad_depth"][~finite])
    assert (np.count_nonzero(vjp["grad_depth"]) > 5) == (softness > 0)
    num = np.zeros((4, 4))
    for r in range(4):
        for j in range(4):
            e = np.zeros((4, 4))
            e[r, j] = h
            num[r, j] = (loss(depth, pos, M + e) - loss(depth, pos, M - e)) / (2 * h)
    assert np.abs(num - vjp["grad_matrix"]).max() <= 1e-6 * scale(vjp["grad_matrix"])
    assert np.count_nonzero(vjp["grad_matrix"]) >= 8
    for r in range(3):
        e = np.zeros(3)
        e[r] = h
        num = (loss(depth, pos + e, M, True) - loss(depth, pos - e, M, True)) / (2 * h)
        assert np.abs(num - vjp["grad_positions"][..., r]).max() <= 1e-6 * scale(vjp["grad_positions"]), r
    assert np.count_nonzero(vjp["grad_positions"]) > 50


# ---- the framework-op statement

def _ops_run(inputs, dtype, unbatched=False):
    depth, pos, M, bias, softness, mask, grad = inputs
    if unbatched:
        pos, grad, mask = pos[0], grad[0], None if mask is None else mask[0]
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True) for a in (depth, pos, M)]
    vis, valid = deferred.sample_shadow(*ts, bias, softness, None if mask is None else torch.from_numpy(mask))
    assert "_SampleShadowFn" not in vis.grad_fn.name() and not valid.requires_grad and valid.dtype == torch.bool
    grads = torch.autograd.grad(vis, ts, torch.from_numpy(grad).to(dtype)[..., None], allow_unused=True)
    return vis.detach().numpy(), valid.numpy(), [None if g is None else g.numpy() for g in grads]


@pytest.mark.parametrize("ident", sc.CASE_IDS)
def test_ops_float64_against_the_statement(ident):
    inputs = sc.case_input(ident)
    depth, pos, M, bias, softness, mask, grad = inputs
    fwd = sc.sample(depth, pos, M, bias, softness, mask, np.float64)
    vjp = sc.sample_vjp(depth, pos, M, grad, fwd)
    vis, valid, grads = _ops_run(inputs, torch.float64)
    assert valid.shape == fwd["valid"].shape + (1,) and np.array_equal(valid[..., 0], fwd["valid"]), ident
    assert vis.shape == valid.shape and np.abs(vis[..., 0] - fwd["visibility"]).max() <= 1e-12, ident
    assert not np.any(vis[..., 0][~fwd["valid"]]) and np.all(vis[..., 0][fwd["valid"] & ~fwd["inside"]] == 1.0)
    assert vis.min() >= 0.0 and vis.max() <= 1.0
    for got, name in zip(grads, ("grad_depth", "grad_positions", "grad_matrix")):
        if got is None:  # without a ramp the depth map is not in the graph
            assert name == "grad_depth" and softness == 0 and not np.any(vjp[name]), (ident, name)
            continue
        assert np.all(np.isfinite(got)), (ident, name)
        assert got.shape == vjp[name].shape, (ident, name)
        assert np.abs(got - vjp[name]).max() <= 1e-12 * max(1.0, np.abs(vjp[name]).max()), (ident, name)
    assert not np.any(grads[1][~fwd["inside"]])


def test_ops_forms_and_double_backward():
    """[H,W,3] positions with a shared map and matrix; float32 on a CPU is the statement too, and since each of its
    lines is one IEEE operation it equals the float32 numpy statement bit for bit; create_graph=True works through
    the framework ops."""
    ident = "15x17-m5x7-ss-ortho-soft-bias-random-mask"
    inputs = sc.case_input(ident)
    fwd = sc.case_forward(ident)
    vis, valid, grads = _ops_run(inputs, torch.float32, unbatched=True)
    assert vis.shape == (15, 17, 1) and valid.shape == (15, 17, 1)
    assert np.array_equal(valid[..., 0], fwd["valid"][0])
    assert np.array_equal(vis[..., 0].view(np.uint32), fwd["visibility"][0].view(np.uint32))
    depth, pos, M, bias, softness, mask, grad = inputs
    ts = [torch.from_numpy(a).double().requires_grad_(True) for a in (depth, pos, M)]
    vis, _ = deferred.sample_shadow(*ts, bias, softness, torch.from_numpy(mask))
    g, = torch.autograd.grad(vis.square().sum(), [ts[2]], create_graph=True)
    gg = torch.autograd.grad(g.square().sum(), ts[:2])
    assert all(bool(torch.isfinite(x).all()) for x in gg) and float(gg[0].abs().max()) > 0


# ---- the convention against geometry

def _quad(x0, x1, z0, z1, y):
    return np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], np.float32)


OCCLUDER = (0.2, 1.0, -0.9, -0.3)  # x0, x1, z0, z1 at height 1 over the floor y = 0: off centre, so a flipped axis shows
LIGHT_HEIGHT = 3.0


def _down_light(kind):
    """a light at (0, 3, 0) looking straight down: light space x' = x, y' = -z, z' = y - 3 (the floor at z' = -3)"""
    view = torch.tensor([[1., 0., 0., 0.], [0., 0., 1., 0.], [0., -1., 0., 0.], [0., 0., -LIGHT_HEIGHT, 1.]])
    if kind == "ortho":  # the box |x'|, |y'| <= 2, -z' from near 0.5 to far 6 onto cz in [-1, 1]
        n, f = 0.5, 6.0
        proj = torch.tensor([[0.5, 0., 0., 0.], [0., 0.5, 0., 0.], [0., 0., -2. / (f - n), 0.],
                             [0., 0., -(f + n) / (f - n), 1.]])
    else:
        proj = matrices.perspective_projection(near=1., far=10., right=0.7, aspect=1.)
    return view @ proj


def _shadow_scene(kind, S=64):
    """-> (world vertices [8,3] tensor, faces, light matrix, the analytic shadow rectangle on the floor, the size of
    a texel on the floor)"""
    world = torch.from_numpy(np.concatenate([_quad(-2.5, 2.5, -2.5, 2.5, 0.0), _quad(*OCCLUDER, 1.0)]))
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=torch.int32)
    k = 1.0 if kind == "ortho" else LIGHT_HEIGHT / (LIGHT_HEIGHT - 1.0)  # the point light magnifies the shadow
    half = 2.0 if kind == "ortho" else 0.7 * LIGHT_HEIGHT
    return world, faces, _down_light(kind), tuple(k * c for c in OCCLUDER), 2.0 * half / S


def _render_depth(world, faces, M, S):
    clip = torch.cat([world, torch.ones_like(world[:, :1])], -1) @ M
    return dp.oracle_render(torch.full((S, S, 1), float("inf")), clip, clip[:, 2:3], faces, S, S, 1)


@pytest.mark.parametrize("kind", ["ortho", "persp"])
@pytest.mark.parametrize("softness", [0.0, 0.05])
def test_floor_shadow_is_the_analytic_rectangle(kind, softness):
    S = 64
    world, faces, M, (x0, x1, z0, z1), texel = _shadow_scene(kind, S)
    depth = _render_depth(world, faces, M, S)
    assert bool(torch.isfinite(depth).all())  # (the floor fills the map)
    xs = torch.linspace(-1.7, 1.7, 96)
    zz, xx = torch.meshgrid(xs, xs, indexing="ij")
    floor = torch.stack([xx, torch.zeros_like(xx), zz], -1)
    vis, valid = deferred.sample_shadow(depth, floor, M, bias=0.02, softness=softness)
    assert bool(valid.all())
    vis = vis[..., 0].numpy()
    x, z = xx.numpy(), zz.numpy()
    margin = texel * (1 + 1e-3)
    shadowed = (x > x0 + margin) & (x < x1 - margin) & (z > z0 + margin) & (z < z1 - margin)
    lit = (x < x0 - margin) | (x > x1 + margin) | (z < z0 - margin) | (z > z1 + margin)
    assert shadowed.sum() > 50 and lit.sum() > 1000 and (~shadowed & ~lit).sum() > 50
    assert np.all(vis[shadowed] == 0.0) and np.all(vis[lit] == 1.0)
    band = vis[~shadowed & ~lit]
    assert band.min() >= 0.0 and band.max() <= 1.0 and ((band > 0) & (band < 1)).any()


@pytest.mark.parametrize("kind", ["ortho", "persp"])
def test_cotangent_on_the_shadow_reaches_the_occluder(kind):
    """With a ramp wider than the occluder's clearance (in clip z) the shadowed floor sits on the ramp, so a
    cotangent on it reaches the depth map's texels and, through the rasteriser's backward, the occluder's vertices."""
    S = 64
    world, faces, M, (x0, x1, z0, z1), texel = _shadow_scene(kind, S)
    world.requires_grad_(True)
    depth = _render_depth(world, faces, M, S)
    clip_z = (torch.cat([world, torch.ones_like(world[:, :1])], -1) @ M)[:, 2].detach()
    clearance = float(clip_z[0] - clip_z[4])  # the floor's clip z minus the occluder's
    assert clearance > 0.1
    xs = torch.linspace(-1.7, 1.7, 96)
    zz, xx = torch.meshgrid(xs, xs, indexing="ij")
    floor = torch.stack([xx, torch.zeros_like(xx), zz], -1)
    vis, _ = deferred.sample_shadow(depth, floor, M, bias=0.02, softness=2.0 * clearance)
    inner = (xx > x0 + 2 * texel) & (xx < x1 - 2 * texel) & (zz > z0 + 2 * texel) & (zz < z1 - 2 * texel)
    on_ramp = vis[..., 0][inner]
    assert inner.sum() > 50 and bool(((on_ramp > 0.2) & (on_ramp < 0.8)).all())
    g, = torch.autograd.grad(torch.where(inner, vis[..., 0], 0.0).sum(), [world])
    assert bool(torch.isfinite(g).all())
    assert float(g[4:, 1].abs().min()) > 0  # every corner of the occluder moves the shadow's depth with its height


# ---- argument checks

def test_value_errors():
    d, p, M = torch.zeros((5, 7, 1)), torch.zeros((2, 4, 6, 3)), torch.eye(4)
    with pytest.raises(ValueError, match="positions must be"):
        deferred.sample_shadow(d, torch.zeros((4, 6, 2)), M)
    with pytest.raises(ValueError, match="positions must be"):
        deferred.sample_shadow(d, torch.zeros((6, 3)), M)
    with pytest.raises(ValueError, match="depth_map must be"):
        deferred.sample_shadow(torch.zeros((5, 7, 2)), p, M)
    with pytest.raises(ValueError, match="depth_map must be"):
        deferred.sample_shadow(torch.zeros((5, 7)), p, M)
    with pytest.raises(ValueError, match="depth_map must be"):
        deferred.sample_shadow(torch.zeros((0, 7, 1)), p, M)
    with pytest.raises(ValueError, match="per-frame depth_map"):
        deferred.sample_shadow(torch.zeros((3, 5, 7, 1)), p, M)
    with pytest.raises(ValueError, match="per-frame depth_map"):
        deferred.sample_shadow(torch.zeros((2, 5, 7, 1)), p[0], M)
    for bad in (torch.zeros((3, 4)), torch.zeros((3, 4, 4)), torch.zeros((16,))):
        with pytest.raises(ValueError, match="light_matrix must be"):
            deferred.sample_shadow(d, p, bad)
    with pytest.raises(ValueError, match="light_matrix must be"):
        deferred.sample_shadow(d, p[0], torch.zeros((2, 4, 4)))
    for bad in (-0.1, float("nan"), float("inf"), torch.zeros(()), "1", True):
        with pytest.raises(ValueError, match="bias must be"):
            deferred.sample_shadow(d, p, M, bias=bad)
        with pytest.raises(ValueError, match="softness must be"):
            deferred.sample_shadow(d, p, M, softness=bad)
    with pytest.raises(ValueError, match="mask of shape"):
        deferred.sample_shadow(d, p, M, mask=torch.zeros((4, 6)))
    # per-frame forms that are fine
    vis, valid = deferred.sample_shadow(torch.zeros((2, 5, 7, 1)), p, torch.eye(4).expand(2, 4, 4))
    assert vis.shape == (2, 4, 6, 1) and valid.shape == (2, 4, 6, 1)


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.dirt_abi_version() == 13  # additions only: no signature or workspace layout changed


def _args(fn, frames=1, Sh=4, Sw=4, B=1, H=4, W=4, matrix_pf=0, bias=0.0, softness=0.0, null=(), workspace=1 << 20):
    """Arguments with every pointer set to a host word (the checks under test return before any HIP call) except
    those named in `null`; the last element keeps the word alive."""
    word = ctypes.c_uint64(0)
    p = lambda name: None if name in null else ctypes.addressof(word)  # noqa: E731
    head = [p("depth_map"), frames, Sh, Sw, p("positions"), None, B, H, W, matrix_pf, p("light_matrix"), bias, softness]
    if fn == "dirt_shadow_sample_fwd":
        return head + [p("visibility"), p("valid"), None], word
    return head + [p("grad_visibility"), p("grad_depth_map"), p("grad_positions"), p("grad_light_matrix"),
                   p("workspace"), workspace, None], word


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.dirt_last_error().decode()  # noqa: E731
    big = _lib.MAX_DIM + 1
    everything = ("depth_map", "positions", "light_matrix", "visibility", "valid", "grad_visibility", "grad_depth_map",
                  "grad_positions", "grad_light_matrix", "workspace")
    for fn in NEW_SYMBOLS[1:]:
        f = getattr(lib, fn)
        for bad, msg in ((dict(B=-1), "non-negative"), (dict(H=0), "height, width"), (dict(W=big), "height, width"),
                         (dict(H=big), "height, width"), (dict(Sh=0), "depth map height, width"),
                         (dict(Sw=big), "depth map height, width"), (dict(Sh=big), "depth map height, width"),
                         (dict(frames=2), "frames"), (dict(frames=0), "frames"),
                         (dict(softness=-0.5), "softness"), (dict(softness=float("nan")), "softness"),
                         (dict(bias=-1.0), "bias"), (dict(bias=float("inf")), "bias")):
            a, _keep = _args(fn, **bad)
            assert f(*a) == _lib.DIRT_EINVAL, (fn, bad)
            assert msg in err() and "shadow_sample" in err(), (fn, bad, err())
        a, _keep = _args(fn, B=0, null=everything)
        assert f(*a) == _lib.DIRT_OK, fn
    required = {"dirt_shadow_sample_fwd": ("depth_map", "positions", "light_matrix", "visibility", "valid"),
                "dirt_shadow_sample_bwd": ("depth_map", "positions", "light_matrix", "grad_visibility")}
    for fn, names in required.items():
        for name in names:
            a, _keep = _args(fn, null=(name,))
            assert getattr(lib, fn)(*a) == _lib.DIRT_EINVAL, (fn, name)
            assert "null pointer" in err(), (fn, name)
    # the matrix's gradient needs its workspace; with no gradient requested there is no work and no error
    a, _keep = _args("dirt_shadow_sample_bwd", null=("workspace",))
    assert lib.dirt_shadow_sample_bwd(*a) == _lib.DIRT_EINVAL and "workspace" in err()
    a, _keep = _args("dirt_shadow_sample_bwd", workspace=8)
    assert lib.dirt_shadow_sample_bwd(*a) == _lib.DIRT_EINVAL and "workspace" in err()
    a, _keep = _args("dirt_shadow_sample_bwd",
                     null=("grad_depth_map", "grad_positions", "grad_light_matrix", "depth_map", "grad_visibility"))
    assert lib.dirt_shadow_sample_bwd(*a) == _lib.DIRT_OK


def test_workspace_grows_with_the_tiles():
    """sixteen floats per 16 x 16 screen tile of every frame"""
    lib = _lib.load()
    size = ctypes.c_size_t(0)

    def ws(B, H, W):
        assert lib.dirt_shadow_sample_workspace(B, H, W, ctypes.byref(size)) == _lib.DIRT_OK
        return size.value

    assert ws(1, 1, 1) == ws(1, 16, 16) == 64
    assert ws(1, 17, 16) == 128 and ws(1, 17, 17) == 256 and ws(3, 17, 17) == 768
    assert ws(0, 4, 4) == 0
    assert ws(1, 264, 256) == 17 * 16 * 64 and ws(2, 8192, 8192) == 2 * 512 * 512 * 64
    assert lib.dirt_shadow_sample_workspace(1, 0, 4, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_shadow_sample_workspace(1, 4, _lib.MAX_DIM + 1, ctypes.byref(size)) == _lib.DIRT_EINVAL
    assert lib.dirt_shadow_sample_workspace(1, 4, 4, None) == _lib.DIRT_EINVAL
