// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after shade_lights_kernels.h.
// Not a standalone header.  It reuses deferred_kernels.h's route accessors, pixel_at, window_max, routed3 and
// ShadeAdjoint, and shade_lights_kernels.h's sl_wave_sum, mul33, kSlThreads / kSlWaves; the forward's opening and the
// gather are written out here as in the shade (DESIGN.md 7k has why).
//
// deferred.shade_pbr: the metallic-roughness model (Lambert + a GGX lobe) under up to DIRT_MAX_LIGHTS directional or
// point lights with a per-pixel, per-light visibility, and gradients to the G-buffers, the material, the visibility,
// the lights, the camera and the ambient colour (DESIGN.md 6i states the rule; tests/shade_pbr_cases.py is the float64
// statement of record).  Dilation, `valid` and the route word are the shade's; colours, material and visibility are
// read at the pixel itself.  For a valid pixel, u(x) = x / (|x| + eps):
//   n = u(n_d)  v = u(cam - p)  l = u(-d_i) or u(q_i - p)  h = u(l + v)
//   r = clamp(material_0, R_MIN, 1)  m = clamp(material_1, 0, 1)  alpha = r r  k = alpha / 2
//   nl = n . l  nv = max(n . v, 0)  nh = n . h  vh = clamp(v . h, 0, 1)
//   t = |n x h|^2 + (nh alpha)^2   D = t > 0 ? alpha^2 / (pi t^2) : 0   V = 1 / (4 (nl (1 - k) + k) (nv (1 - k) + k))
//   F0 = 0.04 + (c - 0.04) m   F = F0 + (1 - F0) (1 - vh)^5
//   term_i = nl > 0 ? vis_i ((lc_i nl) (((1 - F) (1 - m)) (c / pi)) + (lc_i nl) ((D V) F)) : 0
//   acc = term_0;  acc = acc + term_i ...;  pixels = acc + c * ambient
// The cross-product form of t is part of the rule: nh^2 (alpha^2 - 1) + 1 cancels in float32 at low roughness.
//
// Forward: one thread per pixel, a loop over the lights, a branch per light on the mask bit (uniform over the launch).
// Backward, first kernel: a workgroup of kSlThreads owns a chunk of 256 contiguous pixels of ONE frame (grid = chunks
// per frame x min(frames, 65535), a stride loop over the frames), one pixel per thread.  The lights are the outer
// loop: per light a thread adds the light's adjoints of n, v, the colour, alpha and the metallic into its pixel's
// sums, stores the light's visibility gradient, and its six parameter terms (vector 3, colour 3) are reduced across
// the wave by the __shfl_xor butterfly and parked in LDS [wave][column].  After the last light the sums pass through
// u once (n -> the normal, v -> the position and the camera), the six light-independent sums (ambient 3, camera 3)
// follow, one barrier, and threads 0 .. P-1 add the four waves' values in wave order and store the chunk's P = 6 + 6 N
// partial sums to workspace[frame][chunk][P] with plain stores.  Then the own-pixel gradients (colour, material) and
// the G-buffer gather, as the shade's: own adjoint first, then the window in row-major order, a neighbour's adjoint
// recomputed where its route points back (that adds nothing to a parameter: a pixel's parameter terms are counted
// once, by the thread that owns it).
// Backward, second kernel (launched after the first on the same stream; the kernel boundary is the hand-off): one
// workgroup per column of the partial rows, shade_lights_reduce_kernel's shape; a workgroup whose column nobody asked
// for returns.  No float atomics anywhere: every gradient is bit-identical from run to run.  With no parameter
// gradient requested the first kernel is instantiated without the sums, the partials and the LDS, and the second is
// not launched; the two instantiations' other gradients are bit-identical.  All offsets 64-bit.

constexpr int kPbrFixedSums = 6;      // ambient 3, camera 3
constexpr int kPbrSumsPerLight = 6;   // light vector 3, light colour 3
constexpr int kPbrMaxSums = kPbrFixedSums + kPbrSumsPerLight * DIRT_MAX_LIGHTS;
constexpr float kPbrPi = 3.14159265358979323846f;
constexpr float kPbrInvPi = 0.31830988618379067154f;
constexpr float kPbrEps = 1.e-12f;

struct ShadePbrArgs {
    const float *ambient;      // 3 floats, or NULL (zero)
    const float *lvec, *lcol;  // [N, 3], or [B, N, 3] with lights_pf
    const float *cam;          // [3], or [B, 3] with cam_pf
    int n;
    uint32_t point_mask;
    int lights_pf, cam_pf;
};

struct PbrLight {
    float3 v, c;
    bool point;
};
__device__ __forceinline__ PbrLight pbr_light(const ShadePbrArgs &A, int64_t frame, int i)
{
    const int64_t o = ((A.lights_pf ? frame * A.n : 0) + i) * 3;
    PbrLight L;
    L.v = ld3(A.lvec + o);
    L.c = ld3(A.lcol + o);
    L.point = ((A.point_mask >> i) & 1u) != 0;
    return L;
}
__device__ __forceinline__ float3 pbr_camera(const ShadePbrArgs &A, int64_t frame)
{
    return A.n > 0 ? ld3(A.cam + (A.cam_pf ? frame * 3 : 0)) : make_float3(0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ float3 pbr_ambient(const ShadePbrArgs &A)
{
    return A.ambient ? ld3(A.ambient) : make_float3(0.0f, 0.0f, 0.0f);
}

// torch.clamp: a NaN stays a NaN
__device__ __forceinline__ float pbr_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
// J^T g of x -> x / (|x| + eps), m = |x|: the length's subgradient at 0 is 0
__device__ __forceinline__ float3 pbr_unit_vjp(float3 x, float m, float3 g)
{
    const float d = m + kPbrEps;
    float3 r = mul3(g, 1.0f / d);
    if (m > 0.0f) r = sub3(r, mul3(x, dot3(x, g) / (m * d * d)));
    return r;
}

struct PbrPixel {
    float3 pos, nd, col, g;  // dilated position and normal, base colour, upstream gradient
    float rough, metal;      // the material as stored
};
// what the lights of one pixel share
struct PbrSurface {
    float3 n, v, tc, f0, cpi;  // unit normal, unit view vector, cam - p, F0, c / pi
    float nd_m, tc_m;          // |n_d|, |cam - p|
    float m, alpha, k, omk, nvr, gv;
};
__device__ __forceinline__ PbrSurface pbr_surface(const PbrPixel &x, float3 cam)
{
    PbrSurface s;
    s.nd_m = norm3(x.nd);
    s.n = mul3(x.nd, 1.0f / (s.nd_m + kPbrEps));
    s.tc = sub3(cam, x.pos);
    s.tc_m = norm3(s.tc);
    s.v = mul3(s.tc, 1.0f / (s.tc_m + kPbrEps));
    const float r = pbr_clamp(x.rough, DIRT_PBR_MIN_ROUGHNESS, 1.0f);
    s.m = pbr_clamp(x.metal, 0.0f, 1.0f);
    s.alpha = r * r;
    s.k = s.alpha * 0.5f;
    s.omk = 1.0f - s.k;
    s.nvr = dot3(s.n, s.v);
    s.gv = (s.nvr < 0.0f ? 0.0f : s.nvr) * s.omk + s.k;
    s.f0 = make_float3(0.04f + (x.col.x - 0.04f) * s.m, 0.04f + (x.col.y - 0.04f) * s.m,
                       0.04f + (x.col.z - 0.04f) * s.m);
    s.cpi = make_float3(x.col.x / kPbrPi, x.col.y / kPbrPi, x.col.z / kPbrPi);
    return s;
}

// one light's geometry and BRDF factors at one pixel; only `lraw`, `l`, `nl`, `lit` mean anything where !lit
struct PbrLobe {
    bool lit;
    float3 lraw, l, hs, h, xc, F;
    float lraw_m, hs_m, nl, nh, vhr, a, t, D, V, gl, w4, w5;
};
__device__ __forceinline__ PbrLobe pbr_lobe(const PbrPixel &x, const PbrSurface &s, float3 vec, bool point)
{
    PbrLobe o;
    o.lraw = point ? sub3(vec, x.pos) : mul3(vec, -1.0f);
    o.lraw_m = norm3(o.lraw);
    o.l = mul3(o.lraw, 1.0f / (o.lraw_m + kPbrEps));
    o.nl = dot3(s.n, o.l);
    o.lit = o.nl > 0.0f;
    o.hs = add3(o.l, s.v);
    o.hs_m = norm3(o.hs);
    o.h = mul3(o.hs, 1.0f / (o.hs_m + kPbrEps));
    o.nh = dot3(s.n, o.h);
    o.vhr = dot3(s.v, o.h);
    o.xc = cross3(s.n, o.h);
    o.a = o.nh * s.alpha;
    o.t = dot3(o.xc, o.xc) + o.a * o.a;
    o.D = o.t > 0.0f ? (s.alpha * s.alpha) / (kPbrPi * (o.t * o.t)) : 0.0f;
    o.gl = o.nl * s.omk + s.k;
    o.V = 1.0f / (4.0f * (o.gl * s.gv));
    const float w = 1.0f - pbr_clamp(o.vhr, 0.0f, 1.0f), w2 = w * w;
    o.w4 = w2 * w2;
    o.w5 = o.w4 * w;
    o.F = make_float3(s.f0.x + (1.0f - s.f0.x) * o.w5, s.f0.y + (1.0f - s.f0.y) * o.w5,
                      s.f0.z + (1.0f - s.f0.z) * o.w5);
    return o;
}
// d + s per unit of light colour times nl: ((1 - F) (1 - m)) (c / pi) + (D V) F
__device__ __forceinline__ float3 pbr_brdf(const PbrSurface &s, const PbrLobe &o)
{
    const float om = 1.0f - s.m, dv = o.D * o.V;
    return make_float3(((1.0f - o.F.x) * om) * s.cpi.x + dv * o.F.x, ((1.0f - o.F.y) * om) * s.cpi.y + dv * o.F.y,
                       ((1.0f - o.F.z) * om) * s.cpi.z + dv * o.F.z);
}

__global__ __launch_bounds__(kLightThreads) void shade_pbr_fwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals,
    const float *__restrict__ material, const float *__restrict__ visibility, int H, int W, int64_t n, ShadePbrArgs A,
    float *__restrict__ pixels, uint8_t *__restrict__ valid, uint32_t *__restrict__ route)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float3 pos = ld3(positions + p * 3), nv = ld3(normals + p * 3);
    uint32_t r = route_own<6>();
    if (isinf(pos.x) || isinf(pos.y) || isinf(pos.z)) {
        // background: positions and normals both dilate under the positions' mask
        const PixelAt at = pixel_at(p, H, W);
        float mp[3] = {0.0f, 0.0f, 0.0f}, mn[3] = {0.0f, 0.0f, 0.0f};
        r = window_max<3>(positions, at, H, W, mp);
        r |= window_max<3>(normals, at, H, W, mn) << kRouteNormals;
        pos = make_float3(mp[0], mp[1], mp[2]);
        nv = make_float3(mn[0], mn[1], mn[2]);
    }
    const bool ok = finite3(pos) && finite3(nv);
    float3 px = make_float3(0.0f, 0.0f, 0.0f);
    if (ok) {
        const int64_t frame = (A.lights_pf || A.cam_pf) ? p / ((int64_t)H * W) : 0;
        PbrPixel x;
        x.pos = pos;
        x.nd = nv;
        x.col = ld3(colors + p * 3);
        x.g = make_float3(0.0f, 0.0f, 0.0f);
        x.rough = material[p * 2];
        x.metal = material[p * 2 + 1];
        const PbrSurface s = pbr_surface(x, pbr_camera(A, frame));
        float3 acc = make_float3(0.0f, 0.0f, 0.0f);
        for (int i = 0; i < A.n; ++i) {
            const PbrLight L = pbr_light(A, frame, i);
            const PbrLobe o = pbr_lobe(x, s, L.v, L.point);
            float3 term = make_float3(0.0f, 0.0f, 0.0f);
            if (o.lit) {
                const float vis = visibility ? visibility[p * A.n + i] : 1.0f;
                term = mul3(mul33(mul3(L.c, o.nl), pbr_brdf(s, o)), vis);
            }
            acc = i == 0 ? term : add3(acc, term);
        }
        px = add3(acc, mul33(x.col, pbr_ambient(A)));
    }
    st3(pixels + p * 3, px);
    valid[p] = ok ? 1 : 0;
    route[p] = r | (ok ? kRouteValid : 0u);
}

// the sums of one pixel's adjoints over the lights, before n and v pass through u
struct PbrSums {
    float3 n, v, pos, col;  // pos: the point lights' part
    float alpha, metal;
};
__device__ __forceinline__ PbrSums pbr_zero_sums()
{
    PbrSums a;
    a.n = a.v = a.pos = a.col = make_float3(0.0f, 0.0f, 0.0f);
    a.alpha = a.metal = 0.0f;
    return a;
}

// one light's adjoint of one valid pixel, added into `a`; returns the visibility's gradient; with kParams the light's
// six parameter terms (vector 3, colour 3) are added into `t`
template <bool kParams>
__device__ __forceinline__ float pbr_light_adjoint(const PbrPixel &x, const PbrSurface &s, const PbrLight &L, float vis,
                                                   PbrSums &a, float t[kPbrSumsPerLight])
{
    const PbrLobe o = pbr_lobe(x, s, L.v, L.point);
    if (!o.lit) return 0.0f;  // a select: exactly 0, no gradient
    const float om = 1.0f - s.m, dv = o.D * o.V;
    const float3 e = mul3(L.c, o.nl), brdf = pbr_brdf(s, o);
    const float gvis = dot3(x.g, mul33(e, brdf));
    const float3 gt = mul3(x.g, vis);
    const float3 glc = mul33(mul3(gt, o.nl), brdf);
    float gnl = dot3(mul33(gt, L.c), brdf);
    const float3 gb = mul33(gt, e);
    const float3 omf = make_float3(1.0f - o.F.x, 1.0f - o.F.y, 1.0f - o.F.z);
    // brdf = ((1 - F) om) cpi + dv F
    const float gdv = dot3(gb, o.F);
    const float3 gf = make_float3(gb.x * (dv - om * s.cpi.x), gb.y * (dv - om * s.cpi.y), gb.z * (dv - om * s.cpi.z));
    float gm = -dot3(gb, mul33(omf, s.cpi));
    float3 gcol = mul3(mul33(gb, omf), om * kPbrInvPi);
    // F = F0 + (1 - F0) w5, F0 = 0.04 + (c - 0.04) m
    const float3 gf0 = mul3(gf, 1.0f - o.w5);
    const float gw5 = dot3(gf, make_float3(1.0f - s.f0.x, 1.0f - s.f0.y, 1.0f - s.f0.z));
    gcol = add3(gcol, mul3(gf0, s.m));
    gm += dot3(gf0, make_float3(x.col.x - 0.04f, x.col.y - 0.04f, x.col.z - 0.04f));
    const float gvh = (o.vhr >= 0.0f && o.vhr <= 1.0f) ? -(gw5 * 5.0f * o.w4) : 0.0f;
    // D V, V = 1 / (4 gl gv), gl = nl (1 - k) + k, gv = nv (1 - k) + k
    const float gD = gdv * o.V, gV = gdv * o.D;
    const float ggl = -gV * o.V / o.gl, ggv = -gV * o.V / s.gv;
    gnl += ggl * s.omk;
    const float nv = s.nvr < 0.0f ? 0.0f : s.nvr;
    const float gnv = s.nvr >= 0.0f ? ggv * s.omk : 0.0f;
    float gal = ((ggl + ggv) - (ggl * o.nl + ggv * nv)) * 0.5f;
    // D = alpha^2 / (pi t^2), t = xc . xc + a^2, a = nh alpha
    float gtt = 0.0f;
    if (o.t > 0.0f) {
        gal += gD * 2.0f * o.D / s.alpha;
        gtt = -2.0f * o.D / o.t * gD;
    }
    const float3 gx = mul3(o.xc, 2.0f * gtt);
    const float ga = 2.0f * o.a * gtt, gnh = ga * s.alpha;
    gal += ga * o.nh;
    // the vectors
    const float3 gn = add3(add3(cross3(o.h, gx), mul3(o.h, gnh)), add3(mul3(s.v, gnv), mul3(o.l, gnl)));
    const float3 gh = add3(add3(cross3(gx, s.n), mul3(s.n, gnh)), mul3(s.v, gvh));
    const float3 ghs = pbr_unit_vjp(o.hs, o.hs_m, gh);
    const float3 gv = add3(add3(mul3(o.h, gvh), mul3(s.n, gnv)), ghs);
    const float3 gl = add3(mul3(s.n, gnl), ghs);
    const float3 glraw = pbr_unit_vjp(o.lraw, o.lraw_m, gl);
    a.n = add3(a.n, gn);
    a.v = add3(a.v, gv);
    a.col = add3(a.col, gcol);
    a.alpha += gal;
    a.metal += gm;
    if (L.point) a.pos = sub3(a.pos, glraw);  // l = u(q - p): the position receives -, the light's position +
    if (kParams) {
        const float sign = L.point ? 1.0f : -1.0f;
        t[0] += sign * glraw.x;
        t[1] += sign * glraw.y;
        t[2] += sign * glraw.z;
        t[3] += glc.x;
        t[4] += glc.y;
        t[5] += glc.z;
    }
    return gvis;
}

// a valid pixel's adjoints once the lights are summed: the dilated position and normal, the colour, the material, and
// the camera's term
struct PbrOwn {
    ShadeAdjoint a;
    float rough, metal;
    float3 cam;
};
__device__ __forceinline__ PbrOwn pbr_finish(const PbrPixel &x, const PbrSurface &s, const PbrSums &sums, float3 amb)
{
    PbrOwn o;
    o.cam = pbr_unit_vjp(s.tc, s.tc_m, sums.v);
    o.a.pos = sub3(sums.pos, o.cam);
    o.a.nrm = pbr_unit_vjp(x.nd, s.nd_m, sums.n);
    o.a.col = add3(sums.col, mul33(x.g, amb));
    const float r = pbr_clamp(x.rough, DIRT_PBR_MIN_ROUGHNESS, 1.0f);
    o.rough = (x.rough >= DIRT_PBR_MIN_ROUGHNESS && x.rough <= 1.0f) ? 2.0f * r * sums.alpha : 0.0f;
    o.metal = (x.metal >= 0.0f && x.metal <= 1.0f) ? sums.metal : 0.0f;
    return o;
}

__device__ __forceinline__ PbrPixel pbr_load_pixel(const float *__restrict__ positions,
                                                   const float *__restrict__ colors,
                                                   const float *__restrict__ normals,
                                                   const float *__restrict__ material, const float *__restrict__ grad,
                                                   PixelAt at, int H, int W, uint32_t r)
{
    const int64_t q = at.f0 + (int64_t)at.y * W + at.x;
    PbrPixel x;
    x.pos = routed3(positions, at, H, W, r);
    x.nd = routed3(normals, at, H, W, route_normals(r));
    x.col = ld3(colors + q * 3);
    x.g = ld3(grad + q * 3);
    x.rough = material[q * 2];
    x.metal = material[q * 2 + 1];
    return x;
}

// the position and normal adjoints of a valid pixel q that another thread owns: every light in index order
__device__ __forceinline__ ShadeAdjoint pbr_adjoint(const PbrPixel &x, const ShadePbrArgs &A, int64_t frame, int64_t q,
                                                    const float *__restrict__ visibility, float3 cam, float3 amb)
{
    const PbrSurface s = pbr_surface(x, cam);
    PbrSums sums = pbr_zero_sums();
    float unused[kPbrSumsPerLight];
    for (int i = 0; i < A.n; ++i)
        pbr_light_adjoint<false>(x, s, pbr_light(A, frame, i), visibility ? visibility[q * A.n + i] : 1.0f, sums,
                                 unused);
    return pbr_finish(x, s, sums, amb).a;
}

template <bool kParams>
__global__ __launch_bounds__(kSlThreads) void shade_pbr_bwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals,
    const float *__restrict__ material, const float *__restrict__ visibility, int B, int H, int W, ShadePbrArgs A,
    const float *__restrict__ grad, const uint32_t *__restrict__ route, float *__restrict__ grad_positions,
    float *__restrict__ grad_colors, float *__restrict__ grad_normals, float *__restrict__ grad_material,
    float *__restrict__ grad_visibility, float *__restrict__ partial)
{
    __shared__ float wave_sums[kParams ? kSlWaves : 1][kParams ? kPbrMaxSums : 1];
    const int64_t hw = (int64_t)H * W;
    const int chunk = blockIdx.x, chunks = gridDim.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = kPbrFixedSums + kPbrSumsPerLight * A.n;
    const float3 zero = make_float3(0.0f, 0.0f, 0.0f);
    const float3 amb = pbr_ambient(A);
    // (a grid's second dimension holds fewer frames than a batch may have)
    for (int64_t frame = blockIdx.y; frame < B; frame += gridDim.y) {
        const float3 cam = pbr_camera(A, frame);
        const int64_t in_frame = (int64_t)chunk * kSlThreads + tid;
        const bool inside = in_frame < hw;
        PixelAt at;
        at.f0 = frame * hw;
        at.y = inside ? (int)(in_frame / W) : 0;
        at.x = inside ? (int)(in_frame - (int64_t)at.y * W) : 0;
        const int64_t p = at.f0 + (inside ? in_frame : 0);
        const uint32_t r = inside ? route[p] : 0u;
        const bool ok = (r & kRouteValid) != 0;
        PbrPixel x;
        x.pos = x.nd = x.col = x.g = zero;
        x.rough = x.metal = 0.0f;
        if (ok) x = pbr_load_pixel(positions, colors, normals, material, grad, at, H, W, r);
        const PbrSurface s = pbr_surface(x, cam);
        PbrSums sums = pbr_zero_sums();
        for (int i = 0; i < A.n; ++i) {
            const PbrLight L = pbr_light(A, frame, i);
            float t[kPbrSumsPerLight];
#pragma unroll
            for (int j = 0; j < kPbrSumsPerLight; ++j) t[j] = 0.0f;
            float gvis = 0.0f;
            if (ok)
                gvis = pbr_light_adjoint<kParams>(x, s, L, visibility ? visibility[p * A.n + i] : 1.0f, sums, t);
            if (grad_visibility && inside) grad_visibility[p * A.n + i] = gvis;
            if (kParams) {
#pragma unroll
                for (int j = 0; j < kPbrSumsPerLight; ++j) {
                    const float w = sl_wave_sum(t[j]);
                    if (lane == 0) wave_sums[wave][kPbrFixedSums + kPbrSumsPerLight * i + j] = w;
                }
            }
        }
        PbrOwn own;
        own.a.pos = own.a.nrm = own.a.col = own.cam = zero;
        own.rough = own.metal = 0.0f;
        if (ok) own = pbr_finish(x, s, sums, amb);
        if (kParams) {
            const float3 gamb = mul33(x.g, x.col);  // (zero at a pixel that is not valid)
            const float fixed[kPbrFixedSums] = {gamb.x, gamb.y, gamb.z, own.cam.x, own.cam.y, own.cam.z};
#pragma unroll
            for (int j = 0; j < kPbrFixedSums; ++j) {
                const float w = sl_wave_sum(fixed[j]);
                if (lane == 0) wave_sums[wave][j] = w;
            }
            __syncthreads();
            if (tid < P) {
                float w = wave_sums[0][tid];
#pragma unroll
                for (int k = 1; k < kSlWaves; ++k) w += wave_sums[k][tid];
                partial[(frame * chunks + chunk) * P + tid] = w;
            }
            __syncthreads();  // (the next frame of this workgroup writes wave_sums again)
        }
        if (!inside) continue;
        if (grad_colors) st3(grad_colors + p * 3, own.a.col);
        if (grad_material) {
            grad_material[p * 2] = own.rough;
            grad_material[p * 2 + 1] = own.metal;
        }
        if (!grad_positions && !grad_normals) continue;
        // the G-buffer gradients: own term first, then the window in row-major order
        float acc[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[c] = route_code(r, c) == kRouteOwn ? (&own.a.pos.x)[c] : 0.0f;
            acc[3 + c] = route_normal_code(r, c) == kRouteOwn ? (&own.a.nrm.x)[c] : 0.0f;
        }
#pragma unroll 1
        for (int w = 0; w < 9; ++w) {
            const int dy = w / 3 - 1, dx = w - 3 * (w / 3) - 1;
            const int yy = at.y + dy, xx = at.x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const bool self = w == 4;
            const uint32_t back = (uint32_t)(8 - w);  // the neighbour sees this pixel at the mirrored position
            PixelAt aq = at;
            aq.y = yy;
            aq.x = xx;
            const int64_t q = at.f0 + (int64_t)yy * W + xx;
            const uint32_t rq = self ? r : route[q];
            if (!(rq & kRouteValid) || !route_any(rq, 6, back)) continue;
            ShadeAdjoint a = own.a;
            if (!self)
                a = pbr_adjoint(pbr_load_pixel(positions, colors, normals, material, grad, aq, H, W, rq), A, frame, q,
                                visibility, cam, amb);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (route_code(rq, c) == back) acc[c] += (&a.pos.x)[c];
                if (route_normal_code(rq, c) == back) acc[3 + c] += (&a.nrm.x)[c];
            }
        }
        if (grad_positions) st3(grad_positions + p * 3, make_float3(acc[0], acc[1], acc[2]));
        if (grad_normals) st3(grad_normals + p * 3, make_float3(acc[3], acc[4], acc[5]));
    }
}

// where column j of a partial row goes (SlColumn: the output element of frame 0 and the stride between frames)
struct PbrParamGrads {
    float *ambient, *lvec, *lcol, *cam;
};
__device__ __forceinline__ SlColumn pbr_column(int j, int n_lights, int lights_pf, int cam_pf, const PbrParamGrads &G)
{
    SlColumn c = {nullptr, 0};
    if (j < 3) {
        if (G.ambient) c.out = G.ambient + j;
    } else if (j < 6) {
        if (G.cam) c.out = G.cam + (j - 3);
        c.stride = cam_pf ? 3 : 0;
    } else {
        const int i = (j - kPbrFixedSums) / kPbrSumsPerLight, e = (j - kPbrFixedSums) - i * kPbrSumsPerLight;
        float *base = e < 3 ? G.lvec : G.lcol;
        if (base) c.out = base + i * 3 + (e % 3);
        c.stride = lights_pf ? (int64_t)n_lights * 3 : 0;
    }
    return c;
}

__global__ __launch_bounds__(kSlThreads) void shade_pbr_reduce_kernel(const float *__restrict__ partial, int B,
                                                                      int chunks, int n_lights, int lights_pf,
                                                                      int cam_pf, PbrParamGrads G)
{
    __shared__ float wave_sums[kSlWaves];
    const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = kPbrFixedSums + kPbrSumsPerLight * n_lights;
    const SlColumn col = pbr_column(j, n_lights, lights_pf, cam_pf, G);
    if (!col.out) return;  // (the whole workgroup: nobody asked for this column)
    float total = 0.0f;
    for (int64_t frame = 0; frame < B; ++frame) {
        float s = 0.0f;
        for (int64_t c = tid; c < chunks; c += kSlThreads) s += partial[(frame * chunks + c) * P + j];
        s = sl_wave_sum(s);
        if (lane == 0) wave_sums[wave] = s;
        __syncthreads();
        float f = wave_sums[0];
#pragma unroll
        for (int w = 1; w < kSlWaves; ++w) f += wave_sums[w];
        __syncthreads();
        if (col.stride) {
            if (tid == 0) col.out[frame * col.stride] = f;
        } else {
            total = frame == 0 ? f : total + f;
        }
    }
    if (!col.stride && tid == 0) *col.out = total;
}
