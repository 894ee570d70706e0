"""Edge-shape inputs for the lighting helpers, shared by tests/test_lighting_f64.py (framework ops on a CPU) and
tests/test_gpu_lighting_f64.py (fused HIP kernels), with the comparison against tests/lighting_f64.py under the
project's float32 contract (tests/test_gpu_lighting.py): forward within 2e-6 + 1e-5 |ref|, gradients within 1e-4
of the gradient's scale.  numpy only; all inputs float32 (the statement evaluates them in float64).  TEST
INFRASTRUCTURE ONLY.
"""
import numpy as np

import lighting_f64

F32 = np.float32
FWD_ATOL, FWD_RTOL, GRAD_FRAC = 2e-6, 1e-5, 1e-4
BIG_ROW_RTOL = 1e-5  # rows whose gradient is of order 1 / eps (a position on the light): relative, on their own

LD = (np.array([1.0, -0.3, -0.5]) / np.linalg.norm([1.0, -0.3, -0.5])).astype(F32)
LC = np.array([1.0, 0.5, 0.25], F32)
CAM = np.array([0.25, 1.75, 2.25], F32)
LP = np.array([0.5, -1.0, 0.5], F32)

SIZES = [(1, 3), (2, 3), (63, 3), (64, 3), (65, 3), (255, 3), (256, 3), (257, 3), (513, 3), (2, 5, 3), (3, 4, 5, 3)]
SHININESS = [0.0, 0.5, 1.0, 2.0, 2.5, 6.0, 50.0, 0, 1, 2, 6, 50]
OPERANDS = {"diffuse": ("normals", "colors"), "specular": ("positions", "normals", "reflectivities"),
            "point": ("positions", "normals", "colors")}
PARAMS = {"diffuse": ("light_direction", "light_color"),
          "specular": ("light_direction", "light_color", "camera_position"),
          "point": ("light_position", "light_color")}


# ---- comparison (NaN-safe in the sense of tests/test_gpu_parity.py's assert_close_grad)

def _same_nonfinite(got, ref, name):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN pattern differs (%d vs %d in the statement)" % (
        name, np.isnan(got).sum(), np.isnan(ref).sum())
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "%s: inf pattern differs" % name
    return got, ref, np.isfinite(ref)


def _worst(err, bound, fin):
    """max err / bound over the finite reference entries (0 / 0 counts as 0; a NaN error as a failure)"""
    err, bound = err[fin], bound[fin]
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return float(np.inf if np.isnan(ratio).any() else ratio.max())


def fwd_ratio(got, ref, name):
    """Worst error over the forward bound 2e-6 + 1e-5 |ref|; the non-finite patterns must agree."""
    got, ref, fin = _same_nonfinite(got, ref, name)
    with np.errstate(invalid="ignore"):
        return _worst(np.abs(got - ref), FWD_ATOL + FWD_RTOL * np.abs(ref), fin)


def grad_ratio(got, ref, name, rows=None, big_rows=(), frac=GRAD_FRAC, big_rtol=BIG_ROW_RTOL):
    """Worst error over the gradient bound: frac of the scale (max |ref|, at least 1e-6) over the compared rows
    (`rows`: a mask over the leading dimensions, default all); each of `big_rows` against big_rtol of its own
    scale, apart from the others."""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, got.shape, ref.shape)
    if got.ndim > 1:
        got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    keep = np.ones(len(got), bool) if rows is None else np.asarray(rows, bool).reshape(-1).copy()
    worst = 0.0
    for b in big_rows:
        keep[b] = False
        g, r, fin = _same_nonfinite(got[b], ref[b], name)
        worst = max(worst, _worst(np.abs(g - r), np.full(r.shape, big_rtol * np.abs(r[fin]).max(initial=0.0)), fin))
    g, r, fin = _same_nonfinite(got[keep], ref[keep], name)
    scale = max(float(np.abs(r[fin]).max(initial=0.0)), 1e-6)
    with np.errstate(invalid="ignore"):
        return max(worst, _worst(np.abs(g - r), np.full(r.shape, frac * scale), fin))


# ---- elementwise cases

class Case:
    """One call of diffuse_directional / specular_directional / diffuse_point: `operands` ([..., 3] float32, in
    the call's order), `params` (the [3] light parameters, in the call's order), upstream gradient `grad`.
    rows: mask of the rows whose position / normal gradients are compared (None: all; the forward and the colour
    gradient are compared everywhere).  big_rows: see grad_ratio."""

    def __init__(self, ident, fn, operands, params, two, grad, shininess=None, rows=None, big_rows=(), marks=None):
        self.id, self.fn, self.two, self.shininess = ident, fn, two, shininess
        self.operands = [np.ascontiguousarray(x, F32) for x in operands]
        self.params = [np.asarray(x, F32) for x in params]
        self.grad = np.ascontiguousarray(grad, F32)
        self.rows, self.big_rows = rows, tuple(big_rows)
        self.marks = marks or {}  # named row sets the exact assertions use

    def args(self):
        a = list(self.operands) + list(self.params)
        return a + [self.shininess] if self.fn == "specular" else a

    def reference(self):
        """(forward, {operand or parameter name: gradient}) of the float64 statement"""
        fwd, vjp = {"diffuse": (lighting_f64.diffuse_directional, lighting_f64.diffuse_directional_vjp),
                    "specular": (lighting_f64.specular_directional, lighting_f64.specular_directional_vjp),
                    "point": (lighting_f64.diffuse_point, lighting_f64.diffuse_point_vjp)}[self.fn]
        if not hasattr(self, "_ref"):
            self._ref = (fwd(*self.args(), self.two), vjp(*self.args(), self.two, self.grad))
        return self._ref


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _params(fn):
    return {"diffuse": [LD, LC], "specular": [LD, LC, CAM], "point": [LP, LC]}[fn]


def random_case(fn, shape, two, seed=0, shininess=6.0, ident=None):
    rng = np.random.default_rng([seed, len(shape), int(np.prod(shape))])
    n = _unit(rng.standard_normal(shape))
    c = rng.uniform(0.1, 1.0, shape)
    p = rng.uniform(-1.0, 1.0, shape)
    ops = [n, c] if fn == "diffuse" else [p, n, c]
    ident = ident or "%s-%s-%s" % (fn, "x".join(map(str, shape)), "two" if two else "one")
    return Case(ident, fn, ops, _params(fn), two, rng.standard_normal(shape),
                shininess if fn == "specular" else None)


def _cos(fn, ops, params):
    """the clamp's argument per row, float64 (used only to sort rows into front- and back-facing)"""
    ops = [np.asarray(x, np.float64) for x in ops]
    params = [np.asarray(x, np.float64) for x in params]
    if fn == "diffuse":
        return -(ops[0] * params[0]).sum(-1)
    if fn == "point":
        d = ops[0] - params[0]
        return (ops[1] * d).sum(-1) / np.linalg.norm(d, axis=-1)
    n, l = ops[1], params[0]
    r = l - 2.0 * (n * l).sum(-1, keepdims=True) * n
    return (_unit(params[2] - ops[0]) * r).sum(-1)


def size_cases():
    return [random_case(fn, shape, two, seed=1) for fn in OPERANDS for shape in SIZES for two in (True, False)]


def kink_cases():
    """The clamp's argument exactly 0 in float32 on the rows marks['kink'], ordinary rows in between."""
    out = []
    g = np.random.default_rng(3).standard_normal((6, 3))
    col = np.random.default_rng(4).uniform(0.2, 1.0, (6, 3))
    kink = np.array([True, True, False, True, True, False])
    for two in (True, False):
        # n . (-l) with l = (0, 1, 0): every product is a zero
        n = [[1, 0, 0], [0, 0, 1], [0.6, 0.64, 0.48], [-1, 0, 0], [0, 0, -2.5], [0.6, -0.64, 0.48]]
        out.append(Case("diffuse-kink-%s" % ("two" if two else "one"), "diffuse", [n, col], [[0, 1, 0], LC], two, g,
                        marks={"kink": kink}))
        # p - light orthogonal to n: (0, 2, 0) . (1, 0, 0); (1, 0, -1) . (1, 0, 1) = a - a; (0, 0, 4) . (3, -2, 0)
        d = np.array([[0, 2, 0], [1, 0, -1], [0.5, 0.25, 1], [0, 0, 4], [-2, 0, 0], [0.5, -0.25, -1]])
        n = [[1, 0, 0], [1, 0, 1], [0.6, 0.64, 0.48], [3, -2, 0], [0, 0.6, -0.8], [0.6, 0.64, 0.48]]
        out.append(Case("point-kink-%s" % ("two" if two else "one"), "point", [LP + d, n, col], [LP, LC], two, g,
                        marks={"kink": kink}))
        # l = (0, -1, 0), n = (0, 1, 0): r = (0, 1, 0), so cos = t_y / |t| + 1e-12f, which is exactly 0 for
        # t_y = -1e-12f |t| with |t| a power of two (cam - p is exact: cam_y = 0).  In float64 the same inputs
        # give cos = 1e-12 - 1e-12f = 4e-21 > 0: both sides of the kink agree for the exponents used here
        # (k = 2: slope 0 at 0; one-sided k = 1: the gradient passes at 0 as it does above it)
        e = F32(1e-12)
        cam = np.array([1.0, 0.0, -0.5], F32)
        t = np.array([[2, -2 * e, 0], [0, -4 * e, 4], [0.5, 0.25, 1], [-1, -e, 0], [0, -0.5 * e, -0.5], [0.5, 1.5, -1]],
                     np.float64)
        n = [[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0.6, 0.64, 0.48]]
        for k in ((2.0,) if two else (2.0, 1.0)):
            out.append(Case("specular-kink-%s-k%g" % ("two" if two else "one", k), "specular",
                            [cam.astype(np.float64) - t, n, col], [[0, -1, 0], LC, cam], two, g, shininess=k,
                            marks={"kink": kink}))
    return out


def backfacing_cases():
    """double_sided=False with half the rows back-facing (marks['back']), |cos| > 0.05 everywhere."""
    out = []
    for fn, k in (("diffuse", None), ("point", None), ("specular", 6.0), ("specular", 0.5)):
        big = random_case(fn, (400, 3), False, seed=5, shininess=k)
        cos = _cos(fn, big.operands, big.params)
        front, back = np.flatnonzero(cos > 0.05)[:35], np.flatnonzero(cos < -0.05)[:35]
        assert len(front) == 35 and len(back) == 35
        pick = np.stack([front, back], 1).reshape(-1)  # interleaved
        out.append(Case("%s-backfacing%s" % (fn, "" if k is None else "-k%g" % k), fn,
                        [x[pick] for x in big.operands], big.params, False, big.grad[pick], shininess=k,
                        marks={"back": np.arange(70) % 2 == 1}))
    return out


def shininess_cases():
    """Front-facing, back-facing and near-grazing rows (cos = 2^-10 / |t| ~ 1e-3) under every exponent, as float
    and as int.  The rows are built so that cos carries no cancellation in float32 (l = (0, 0, -1) and
    n = (0, 0, 1) give r = (0, 0, 1), cos = t_z / |t|, and p = cam - t is exact): an error of 1e-7 in a cos of
    1e-3 is 1e-4 of it, which an exponent below 1 passes straight into the gradient, and an exponent of 50
    multiplies the forward's relative error by 50 -- past the contract for ANY float32 evaluation, this one's
    reference included."""
    cam = np.array([0.5, 1.5, 2.0], F32)
    z = 2.0 ** -10
    t = np.array([[0, 0, 1], [0.5, 0, 1], [0.25, -0.5, 1.5], [-0.125, 0.25, 2],  # front
                  [0.5, 0.25, -1], [0, 0, -2], [-1, 0.5, -0.25],                 # back
                  [1, 0.5, z], [-0.75, 1, z], [0, -2, 2 * z],                    # grazing
                  [0.5, 0.5, 1.0], [0.25, 0.75, -0.5]])                          # tilted normals, front / back
    n = np.tile([0.0, 0.0, 1.0], (len(t), 1))
    n[10], n[11] = _unit(np.array([0.25, 0.125, 1.0])), _unit(np.array([-0.25, 0.5, 1.0]))
    cos = _cos("specular", [cam.astype(np.float64) - t, n, n], [[0, 0, -1], LC, cam])
    assert np.all(cos[4:7] < -0.1) and np.all(np.abs(cos) > 5e-4)
    marks = {"back": cos < 0}
    rng = np.random.default_rng(6)
    refl, g = rng.uniform(0.2, 1.0, t.shape), rng.standard_normal(t.shape)
    out = []
    for k in SHININESS:
        for two in (True, False):
            out.append(Case("specular-shininess-%s%g-%s" % ("int" if isinstance(k, int) else "float", k,
                                                            "two" if two else "one"), "specular",
                            [cam.astype(np.float64) - t, n, refl], [[0, 0, -1], LC, cam], two, g, shininess=k,
                            marks=marks))
    return out


def on_light_cases():
    """diffuse_point with row 2 exactly on the light: its one-sided position gradient is grad / eps ~ 1e12."""
    out = []
    for two in (True, False):
        c = random_case("point", (5, 3), two, seed=7, ident="point-on-light-%s" % ("two" if two else "one"))
        c.operands[0][2] = LP
        c.big_rows = (2,)
        out.append(c)
    return out


def nonfinite_cases():
    """NaN, +inf and -inf in single rows of the normals and positions; the other rows finite (Case.rows)."""
    out = []
    bad = [(1, 0, np.nan), (3, 1, np.inf), (6, 2, -np.inf), (8, 1, np.nan), (10, 0, -np.inf)]  # (row, column, value)
    for fn in OPERANDS:
        for two in (True, False):
            c = random_case(fn, (12, 3), two, seed=8, ident="%s-nonfinite-%s" % (fn, "two" if two else "one"))
            rows = np.ones(12, bool)
            for i, (row, col, val) in enumerate(bad):
                which = 0 if fn == "diffuse" else i % 2  # normals only, or positions and normals in turn
                c.operands[which][row, col] = val
                rows[row] = False
            c.rows = rows
            out.append(c)
    return out


def elementwise_cases():
    return (size_cases() + kink_cases() + backfacing_cases() + shininess_cases() + on_light_cases() +
            nonfinite_cases())


# ---- meshes for vertex_normals

class Mesh:
    """vertices [V, 3] float32 as a function of the frame number (different geometry per frame), faces [F, 3]
    int64 (cast by the tests), zero_g: vertices whose upstream gradient is set to 0."""

    def __init__(self, ident, build, faces, zero_g=(), marks=None):
        self.id, self.build, self.faces = ident, build, np.asarray(faces, np.int64).reshape(-1, 3)
        self.zero_g, self.marks = tuple(zero_g), marks or {}

    def vertices(self, layout):
        """layout 'v3': [V, 3]; 'v4': [V, 4] (w = 1 + a ramp, never read); 'b3': [3, V, 3]"""
        if layout == "b3":
            return np.stack([self.build(k) for k in range(3)]).astype(F32)
        v = self.build(0).astype(F32)
        if layout == "v4":
            v = np.concatenate([v, 1.0 + 0.1 * np.arange(len(v), dtype=F32)[:, None]], 1).astype(F32)
        return v

    def grad(self, layout):
        v = self.vertices(layout)
        g = np.random.default_rng(11).standard_normal(v.shape[:-1] + (3,)).astype(F32)
        g[..., list(self.zero_g), :] = 0
        return g


def _grid(k, n=4):
    u, v = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    y = 0.2 * np.sin(3 * u + 0.5 * k) * np.cos(2 * v) + 0.05 * k * u * v
    return np.stack([u, y, v], -1).reshape(-1, 3)


def _grid_faces(n=4):
    r = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    return np.stack([np.stack([r, r + n, r + 1], -1), np.stack([r + 1, r + n, r + n + 1], -1)], 1).reshape(-1, 3)


def _strip(F):
    i = np.arange(F)
    faces = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1))

    def build(k):
        j = np.arange(F + 2)
        return np.stack([0.5 * j, (j % 2) * (1.0 + 0.25 * k), 0.3 * np.sin(0.7 * j + k)], 1)
    return Mesh("strip%d" % F, build, faces)


def _fan(valence=512):
    """A cone: the hub (vertex 0) is the apex over a ring of `valence` vertices, so the faces' normals all lean
    the same way and their sum at the hub does not cancel.  The faces are slivers (two edges of length ~1.4 at
    an angle of 2 pi / valence), so (v1 - v0) x (v2 - v0) cancels to 1 / 80 of its products: the ring lies in
    z = 0 and the apex height is a power of two, which keeps those products exact in float32 -- any other height
    costs every float32 evaluation 3e-6 on the ring's normals (measured with the framework ops), over a third of
    the contract."""
    i = np.arange(valence)
    faces = np.stack([np.zeros(valence, np.int64), 1 + i, 1 + (i + 1) % valence], 1)

    def build(k):
        th = 2 * np.pi * i / valence
        rad = 1.0 + 0.05 * k * np.sin(3 * th)
        ring = np.stack([rad * np.cos(th), rad * np.sin(th), np.zeros(valence)], 1)
        return np.concatenate([[[0.0, 0.0, 2.0 ** k]], ring])
    return Mesh("fan%d" % valence, build, faces)


def _with_extra(extra):
    return lambda k: np.concatenate([_grid(k), np.asarray(extra, np.float64)])


def mesh_cases():
    single = Mesh("single", lambda k: np.array([[0, 0, 0], [1, 0.25 * k, 0], [0.25, 1, 0.5 + k]], np.float64),
                  [[0, 1, 2]])
    unref = Mesh("unreferenced", _with_extra([[0.3, 0.7, -0.2], [5, 5, 5], [0, 0, 0]]), _grid_faces(),
                 marks={"unreferenced": (16, 17, 18)})
    # a repeated-index face and an exactly collinear one: both normals are exactly 0, so they add nothing; with a
    # zero upstream gradient on the vertices they touch, their backward is 0 / eps = 0 too
    degenerate = Mesh("degenerate", _with_extra([[0, 0, 0], [1, 0, 0], [2, 0, 0]]),
                      np.concatenate([_grid_faces()[:9], [[5, 5, 6], [16, 17, 18]], _grid_faces()[9:]]),
                      zero_g=(5, 6, 16, 17, 18))
    return [single, _strip(255), _strip(256), _strip(257), _fan(512), unref, degenerate]


def out_of_range_faces(dtype):
    """(faces with out-of-range rows mixed into the grid's, the grid's own faces): V = 16"""
    good = _grid_faces()
    bad = [[-1, 0, 1], [0, 16, 1], [0, 1, 2 ** 31 - 1]]
    if dtype == np.int64:
        bad += [[2 ** 40, 0, 1], [4, 5, -2 ** 40]]
    faces = np.concatenate([good[:5], bad[:2], good[5:], bad[2:]]).astype(dtype)
    return faces, good.astype(dtype)


def many_frames(B=70000):
    """(vertices [B, 3, 3], upstream gradient): one triangle per frame, more frames than a grid's y extent holds"""
    rng = np.random.default_rng(12)
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) + 0.1 * rng.standard_normal((B, 3, 3))
    return x.astype(F32), rng.standard_normal((B, 3, 3)).astype(F32)


def grid_mesh():
    return Mesh("grid", _grid, _grid_faces())
