// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after shade_pbr_kernels.h and
// shade_sh_kernels.h.  Not a standalone header.  It reuses deferred_kernels.h's route accessors, pixel_at, window_max,
// routed3 and ShadeAdjoint, shade_lights_kernels.h's sl_wave_sum, mul33, kSlThreads / kSlWaves and SlColumn,
// shade_pbr_kernels.h's pbr_clamp, pbr_unit_vjp and kPbrEps, and shade_sh_kernels.h's basis, order of additions and
// adjoint (ShCoeffs, sh_coeffs, sh_direction, sh_basis, sh_irradiance, sh_adjoint).  The forwards' opening and the
// gather are helpers of this header alone (env_dilated, env_gather), shared by its two ops; the older kernels keep
// theirs written out (DESIGN.md 7k has why), and their listings are untouched.
//
// The two steps that join shade_sh, sample_cubemap_mip and shade_pbr into image-based lighting (DESIGN.md 6j states the
// rules; tests/shade_env_cases.py is the float64 statement of record).  Dilation of positions and normals under the
// positions' background, `valid` and the route word are the shade's.  u(x) = x / (|x| + eps).
//
// deferred.reflect_view: the reflection of the view vector about the normal.  For a valid pixel
//   n = u(n_d)   v = u(cam - p)   nvr = n . v   t = 2 nvr   R = t n - v
// and exactly (0, 0, 0) elsewhere (a direction both cube-map lookups leave out).
//
// deferred.shade_env: the split-sum combination.  colours, material, radiance and occlusion are read at the pixel
// itself.  For a valid pixel
//   n = u(n_d)   v = u(cam - p)   nv = max(n . v, 0)
//   r = clamp(material_0, R_MIN, 1)   m = clamp(material_1, 0, 1)
//   E = shade_sh's irradiance at n (normalize = true)
//   F0 = 0.04 + (c - 0.04) m
//   x = 1 - r   y = 0.0425 - 0.0275 r   z = 1.04 - 0.572 r   w = 0.022 r - 0.04
//   e = exp2(-9.28 nv)   q = x x   s = q < e ? q : e   a = s x + y   A = z - 1.04 a   B = 1.04 a + w
//   S = F0 A + B   dif = ((1 - m) c) E   spec = radiance S   pixels = occlusion (dif + spec)
// dif is shade_sh's pixel with the colour (1 - m) c and the cotangent occlusion g: its adjoints (that colour's, the
// coefficient terms' factor gE, the dilated normal's through u) are sh_adjoint's.
//
// Forwards: one thread per pixel; shade_env templated on K.  Backwards, first kernel: a workgroup of kSlThreads owns a
// chunk of 256 contiguous pixels of ONE frame (grid = chunks per frame x min(frames, 65535), a stride loop over the
// frames), one pixel per thread.  A thread forms its pixel's adjoint; its P parameter terms (camera 3, then for
// shade_env the 3 K coefficient terms in index order) are reduced across the wave by the __shfl_xor butterfly, parked
// in LDS [wave][column], added in wave order by threads 0 .. P-1 and stored to workspace[frame][chunk][P] with plain
// stores.  Then the own-pixel gradients and the G-buffer gather, as the shade's: own adjoint first, then the window in
// row-major order, a neighbour's adjoint recomputed where its route points back (that adds nothing to a parameter).
// Second kernel (launched after the first on the same stream): one workgroup per column of the partial rows,
// shade_lights_reduce_kernel's shape; a workgroup whose column nobody asked for returns.  No float atomics: every
// gradient is bit-identical from run to run.  With no parameter gradient requested the first kernel is instantiated
// without the sums, the partials and the LDS, and the second is not launched; the two instantiations' other gradients
// are bit-identical.  All offsets 64-bit.

constexpr int kEnvCamSums = 3;
constexpr int kEnvMaxSums = kEnvCamSums + 3 * DIRT_MAX_SH_COEFFS;
constexpr float kEnvLn2 = 0.69314718055994530942f;

struct ShadeEnvArgs {
    const float *cam;  // [3], or [B, 3] with cam_pf
    int cam_pf;
    ShadeShArgs sh;    // the coefficients (reflect_view: unused); normalize is set
};

__device__ __forceinline__ float3 env_camera(const ShadeEnvArgs &A, int64_t frame)
{
    return ld3(A.cam + (A.cam_pf ? frame * 3 : 0));
}

// the opening both forwards share with the shade: the dilated position and normal and the route word of pixel p
__device__ __forceinline__ uint32_t env_dilated(const float *__restrict__ positions, const float *__restrict__ normals,
                                                int64_t p, int H, int W, float3 &pos, float3 &nv)
{
    pos = ld3(positions + p * 3);
    nv = ld3(normals + p * 3);
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
    return r;
}

// the unit normal and view vector of one pixel
struct EnvView {
    float3 n, v, tc;    // u(n_d), u(cam - p), cam - p
    float nd_m, tc_m;   // |n_d|, |cam - p|
    float nvr;          // n . v, not clamped
};
__device__ __forceinline__ EnvView env_view(float3 pos, float3 nd, float3 cam)
{
    EnvView s;
    s.nd_m = norm3(nd);
    s.n = sh_direction(nd, true);
    s.tc = sub3(cam, pos);
    s.tc_m = norm3(s.tc);
    s.v = mul3(s.tc, 1.0f / (s.tc_m + kPbrEps));
    s.nvr = dot3(s.n, s.v);
    return s;
}

// the gather both backwards end with: own term first, then the 3x3 window in row-major order; adjoint(aq, rq) is the
// adjoint of the valid neighbour at aq whose route word is rq
template <class F>
__device__ __forceinline__ void env_gather(const uint32_t *__restrict__ route, PixelAt at, int H, int W, uint32_t r,
                                           const ShadeAdjoint &own, F adjoint, float acc[6])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        acc[c] = route_code(r, c) == kRouteOwn ? (&own.pos.x)[c] : 0.0f;
        acc[3 + c] = route_normal_code(r, c) == kRouteOwn ? (&own.nrm.x)[c] : 0.0f;
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
        const uint32_t rq = self ? r : route[at.f0 + (int64_t)yy * W + xx];
        if (!(rq & kRouteValid) || !route_any(rq, 6, back)) continue;
        ShadeAdjoint a = own;
        if (!self) a = adjoint(aq, rq);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (route_code(rq, c) == back) acc[c] += (&a.pos.x)[c];
            if (route_normal_code(rq, c) == back) acc[3 + c] += (&a.nrm.x)[c];
        }
    }
}

// one chunk's P wave-reduced sums, parked by lane 0 of each wave in wave_sums[wave][column]: added in wave order and
// stored to the chunk's partial row
template <int kColumns>
__device__ __forceinline__ void env_store_partial(float (*wave_sums)[kColumns], int P, int tid, float *partial_row)
{
    __syncthreads();
    if (tid < P) {
        float w = wave_sums[0][tid];
#pragma unroll
        for (int k = 1; k < kSlWaves; ++k) w += wave_sums[k][tid];
        partial_row[tid] = w;
    }
    __syncthreads();  // (the next frame of this workgroup writes wave_sums again)
}

// ---- reflect_view

__global__ __launch_bounds__(kLightThreads) void reflect_view_fwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ normals, int H, int W, int64_t n, ShadeEnvArgs A,
    float *__restrict__ directions, uint8_t *__restrict__ valid, uint32_t *__restrict__ route)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float3 pos, nd;
    const uint32_t r = env_dilated(positions, normals, p, H, W, pos, nd);
    const bool ok = finite3(pos) && finite3(nd);
    float3 dir = make_float3(0.0f, 0.0f, 0.0f);
    if (ok) {
        const EnvView s = env_view(pos, nd, env_camera(A, A.cam_pf ? p / ((int64_t)H * W) : 0));
        const float t = 2.0f * s.nvr;
        dir = sub3(mul3(s.n, t), s.v);
    }
    st3(directions + p * 3, dir);
    valid[p] = ok ? 1 : 0;
    route[p] = r | (ok ? kRouteValid : 0u);
}

// the adjoints of one valid pixel's dilated position and normal, and the camera's term
struct ReflectOwn {
    ShadeAdjoint a;  // (col unused)
    float3 cam;
};
__device__ __forceinline__ ReflectOwn reflect_adjoint(float3 pos, float3 nd, float3 g, float3 cam)
{
    const EnvView s = env_view(pos, nd, cam);
    // R = t n - v, t = 2 (n . v)
    const float gnvr = 2.0f * dot3(g, s.n);
    const float3 gn = add3(mul3(g, 2.0f * s.nvr), mul3(s.v, gnvr));
    const float3 gv = sub3(mul3(s.n, gnvr), g);
    ReflectOwn o;
    o.cam = pbr_unit_vjp(s.tc, s.tc_m, gv);
    o.a.pos = mul3(o.cam, -1.0f);
    o.a.nrm = pbr_unit_vjp(nd, s.nd_m, gn);
    o.a.col = make_float3(0.0f, 0.0f, 0.0f);
    return o;
}

template <bool kParams>
__global__ __launch_bounds__(kSlThreads) void reflect_view_bwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ normals, int B, int H, int W, ShadeEnvArgs A,
    const float *__restrict__ grad, const uint32_t *__restrict__ route, float *__restrict__ grad_positions,
    float *__restrict__ grad_normals, float *__restrict__ partial)
{
    __shared__ float wave_sums[kParams ? kSlWaves : 1][kEnvCamSums];
    const int64_t hw = (int64_t)H * W;
    const int chunk = blockIdx.x, chunks = gridDim.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float3 zero = make_float3(0.0f, 0.0f, 0.0f);
    const int64_t in_frame = (int64_t)chunk * kSlThreads + tid;
    const bool inside = in_frame < hw;
    // (a grid's second dimension holds fewer frames than a batch may have)
    for (int64_t frame = blockIdx.y; frame < B; frame += gridDim.y) {
        const float3 cam = env_camera(A, frame);
        PixelAt at;
        at.f0 = frame * hw;
        at.y = inside ? (int)(in_frame / W) : 0;
        at.x = inside ? (int)(in_frame - (int64_t)at.y * W) : 0;
        const int64_t p = at.f0 + (inside ? in_frame : 0);
        const uint32_t r = inside ? route[p] : 0u;
        const bool ok = (r & kRouteValid) != 0;
        ReflectOwn own;
        own.a.pos = own.a.nrm = own.a.col = own.cam = zero;
        if (ok)
            own = reflect_adjoint(routed3(positions, at, H, W, r), routed3(normals, at, H, W, route_normals(r)),
                                  ld3(grad + p * 3), cam);
        if (kParams) {
#pragma unroll
            for (int j = 0; j < kEnvCamSums; ++j) {
                const float w = sl_wave_sum((&own.cam.x)[j]);
                if (lane == 0) wave_sums[wave][j] = w;
            }
            env_store_partial<kEnvCamSums>(wave_sums, kEnvCamSums, tid,
                                           partial + (frame * chunks + chunk) * kEnvCamSums);
        }
        if (!inside || (!grad_positions && !grad_normals)) continue;
        float acc[6];
        env_gather(route, at, H, W, r, own.a,
                   [&](PixelAt aq, uint32_t rq) {
                       const int64_t q = aq.f0 + (int64_t)aq.y * W + aq.x;
                       return reflect_adjoint(routed3(positions, aq, H, W, rq),
                                              routed3(normals, aq, H, W, route_normals(rq)), ld3(grad + q * 3), cam)
                           .a;
                   },
                   acc);
        if (grad_positions) st3(grad_positions + p * 3, make_float3(acc[0], acc[1], acc[2]));
        if (grad_normals) st3(grad_normals + p * 3, make_float3(acc[3], acc[4], acc[5]));
    }
}

// ---- shade_env

struct EnvPixel {
    float3 pos, nd, col, rad, g;  // dilated position and normal, base colour, radiance, upstream gradient
    float rough, metal, occ;      // the material as stored, the occlusion
};

// the environment BRDF's two factors at one pixel, and what their adjoints need
struct EnvBrdf {
    float r, m, x, e, q, s, A, B;
    float3 f0;
};
__device__ __forceinline__ EnvBrdf env_brdf(const EnvPixel &px, float nvr)
{
    EnvBrdf b;
    const float nv = nvr < 0.0f ? 0.0f : nvr;
    b.r = pbr_clamp(px.rough, DIRT_PBR_MIN_ROUGHNESS, 1.0f);
    b.m = pbr_clamp(px.metal, 0.0f, 1.0f);
    b.f0 = make_float3(0.04f + (px.col.x - 0.04f) * b.m, 0.04f + (px.col.y - 0.04f) * b.m,
                       0.04f + (px.col.z - 0.04f) * b.m);
    b.x = 1.0f - b.r;
    const float y = 0.0425f - 0.0275f * b.r, z = 1.04f - 0.572f * b.r, w = 0.022f * b.r - 0.04f;
    b.e = exp2f(-9.28f * nv);
    b.q = b.x * b.x;
    b.s = b.q < b.e ? b.q : b.e;
    const float a = b.s * b.x + y;
    b.A = z - 1.04f * a;
    b.B = 1.04f * a + w;
    return b;
}
// S = F0 A + B;  kd = (1 - m) c
__device__ __forceinline__ float3 env_specular_factor(const EnvBrdf &b)
{
    return make_float3(b.f0.x * b.A + b.B, b.f0.y * b.A + b.B, b.f0.z * b.A + b.B);
}
__device__ __forceinline__ float3 env_diffuse_colour(const EnvPixel &px, const EnvBrdf &b)
{
    return mul3(px.col, 1.0f - b.m);
}

template <int K>
__global__ __launch_bounds__(kLightThreads) void shade_env_fwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals,
    const float *__restrict__ material, const float *__restrict__ radiance, const float *__restrict__ occlusion, int H,
    int W, int64_t n, ShadeEnvArgs A, float *__restrict__ pixels, uint8_t *__restrict__ valid,
    uint32_t *__restrict__ route)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float3 pos, nd;
    const uint32_t r = env_dilated(positions, normals, p, H, W, pos, nd);
    const bool ok = finite3(pos) && finite3(nd);
    float3 out = make_float3(0.0f, 0.0f, 0.0f);
    if (ok) {
        const int64_t frame = (A.cam_pf || A.sh.per_frame) ? p / ((int64_t)H * W) : 0;
        EnvPixel px;
        px.col = ld3(colors + p * 3);
        px.rad = ld3(radiance + p * 3);
        px.rough = material[p * 2];
        px.metal = material[p * 2 + 1];
        px.occ = occlusion ? occlusion[p] : 1.0f;
        const EnvView s = env_view(pos, nd, env_camera(A, frame));
        const EnvBrdf b = env_brdf(px, s.nvr);
        const ShCoeffs<K> C = sh_coeffs<K>(A.sh, frame);
        float Y[K];
        sh_basis<K>(s.n, Y);
        const float3 dif = mul33(env_diffuse_colour(px, b), sh_irradiance<K>(C, Y));
        const float3 spec = mul33(px.rad, env_specular_factor(b));
        out = mul3(add3(dif, spec), px.occ);
    }
    st3(pixels + p * 3, out);
    valid[p] = ok ? 1 : 0;
    route[p] = r | (ok ? kRouteValid : 0u);
}

// a valid pixel's adjoints: the dilated position and normal and the colour (a), the radiance, the material, the
// occlusion, the camera's term, and gE: the coefficient term of (k, c) is gE_c Y_k
struct EnvOwn {
    ShadeAdjoint a;
    float3 rad, cam, gE;
    float rough, metal, occ;
};
template <int K>
__device__ __forceinline__ EnvOwn env_adjoint(const EnvPixel &px, float3 cam, const ShCoeffs<K> &C, float Y[K])
{
    const EnvView s = env_view(px.pos, px.nd, cam);
    const EnvBrdf b = env_brdf(px, s.nvr);
    const float3 kd = env_diffuse_colour(px, b), S = env_specular_factor(b);
    const float3 gt = mul3(px.g, px.occ);
    // dif = kd E(u(n_d)): shade_sh's adjoint with the colour kd
    const ShAdjoint sh = sh_adjoint<K>(px.nd, kd, gt, C, true, Y);
    EnvOwn o;
    o.gE = sh.gE;
    {
        const float3 E = sh_irradiance<K>(C, Y);
        o.occ = dot3(px.g, add3(mul33(kd, E), mul33(px.rad, S)));
    }
    o.rad = mul33(gt, S);
    // kd = (1 - m) c;  S = F0 A + B;  F0 = 0.04 + (c - 0.04) m
    const float3 gS = mul33(gt, px.rad), gf0 = mul3(gS, b.A);
    const float gA = dot3(gS, b.f0), gB = (gS.x + gS.y) + gS.z;
    o.a.col = add3(mul3(sh.col, 1.0f - b.m), mul3(gf0, b.m));
    const float gm = dot3(gf0, make_float3(px.col.x - 0.04f, px.col.y - 0.04f, px.col.z - 0.04f)) -
                     dot3(sh.col, px.col);
    // A = z - 1.04 a, B = 1.04 a + w, a = s x + y, s = q < e ? q : e, q = x x, e = exp2(-9.28 nv)
    const float ga = 1.04f * (gB - gA);
    const float gs = ga * b.x;
    const bool on_q = b.q < b.e;
    const float gx = ga * b.s + (on_q ? 2.0f * b.x * gs : 0.0f);
    const float gnv = on_q ? 0.0f : gs * b.e * (-9.28f * kEnvLn2);
    const float gr = (0.022f * gB - 0.572f * gA) - 0.0275f * ga - gx;
    o.rough = (px.rough >= DIRT_PBR_MIN_ROUGHNESS && px.rough <= 1.0f) ? gr : 0.0f;
    o.metal = (px.metal >= 0.0f && px.metal <= 1.0f) ? gm : 0.0f;
    // nv = max(n . v, 0): the gradient passes where n . v >= 0
    const float gnvr = s.nvr >= 0.0f ? gnv : 0.0f;
    o.cam = pbr_unit_vjp(s.tc, s.tc_m, mul3(s.n, gnvr));
    o.a.pos = mul3(o.cam, -1.0f);
    o.a.nrm = add3(sh.nrm, pbr_unit_vjp(px.nd, s.nd_m, mul3(s.v, gnvr)));
    return o;
}

__device__ __forceinline__ EnvPixel env_load_pixel(const float *__restrict__ positions,
                                                   const float *__restrict__ colors,
                                                   const float *__restrict__ normals,
                                                   const float *__restrict__ material,
                                                   const float *__restrict__ radiance,
                                                   const float *__restrict__ occlusion, const float *__restrict__ grad,
                                                   PixelAt at, int H, int W, uint32_t r)
{
    const int64_t q = at.f0 + (int64_t)at.y * W + at.x;
    EnvPixel px;
    px.pos = routed3(positions, at, H, W, r);
    px.nd = routed3(normals, at, H, W, route_normals(r));
    px.col = ld3(colors + q * 3);
    px.rad = ld3(radiance + q * 3);
    px.g = ld3(grad + q * 3);
    px.rough = material[q * 2];
    px.metal = material[q * 2 + 1];
    px.occ = occlusion ? occlusion[q] : 1.0f;
    return px;
}

template <int K, bool kParams>
__global__ __launch_bounds__(kSlThreads) void shade_env_bwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals,
    const float *__restrict__ material, const float *__restrict__ radiance, const float *__restrict__ occlusion, int B,
    int H, int W, ShadeEnvArgs A, const float *__restrict__ grad, const uint32_t *__restrict__ route,
    float *__restrict__ grad_positions, float *__restrict__ grad_colors, float *__restrict__ grad_normals,
    float *__restrict__ grad_material, float *__restrict__ grad_radiance, float *__restrict__ grad_occlusion,
    float *__restrict__ partial)
{
    __shared__ float wave_sums[kParams ? kSlWaves : 1][kEnvMaxSums];
    constexpr int P = kEnvCamSums + 3 * K;
    const int64_t hw = (int64_t)H * W;
    const int chunk = blockIdx.x, chunks = gridDim.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float3 zero = make_float3(0.0f, 0.0f, 0.0f);
    const int64_t in_frame = (int64_t)chunk * kSlThreads + tid;
    const bool inside = in_frame < hw;
    // (a grid's second dimension holds fewer frames than a batch may have)
    for (int64_t frame = blockIdx.y; frame < B; frame += gridDim.y) {
        const float3 cam = env_camera(A, frame);
        const ShCoeffs<K> C = sh_coeffs<K>(A.sh, frame);
        PixelAt at;
        at.f0 = frame * hw;
        at.y = inside ? (int)(in_frame / W) : 0;
        at.x = inside ? (int)(in_frame - (int64_t)at.y * W) : 0;
        const int64_t p = at.f0 + (inside ? in_frame : 0);
        const uint32_t r = inside ? route[p] : 0u;
        const bool ok = (r & kRouteValid) != 0;
        EnvOwn own;
        own.a.pos = own.a.nrm = own.a.col = own.rad = own.cam = own.gE = zero;
        own.rough = own.metal = own.occ = 0.0f;
        float Y[K];
#pragma unroll
        for (int k = 0; k < K; ++k) Y[k] = 0.0f;
        if (ok)
            own = env_adjoint<K>(
                env_load_pixel(positions, colors, normals, material, radiance, occlusion, grad, at, H, W, r), cam, C,
                Y);
        if (kParams) {
#pragma unroll
            for (int j = 0; j < kEnvCamSums; ++j) {
                const float w = sl_wave_sum((&own.cam.x)[j]);
                if (lane == 0) wave_sums[wave][j] = w;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float w = sl_wave_sum(ok ? (&own.gE.x)[c] * Y[k] : 0.0f);
                    if (lane == 0) wave_sums[wave][kEnvCamSums + 3 * k + c] = w;
                }
            }
            env_store_partial<kEnvMaxSums>(wave_sums, P, tid, partial + (frame * chunks + chunk) * P);
        }
        if (!inside) continue;
        if (grad_colors) st3(grad_colors + p * 3, own.a.col);
        if (grad_material) {
            grad_material[p * 2] = own.rough;
            grad_material[p * 2 + 1] = own.metal;
        }
        if (grad_radiance) st3(grad_radiance + p * 3, own.rad);
        if (grad_occlusion) grad_occlusion[p] = own.occ;
        if (!grad_positions && !grad_normals) continue;
        float acc[6];
        env_gather(route, at, H, W, r, own.a,
                   [&](PixelAt aq, uint32_t rq) {
                       float unused[K];
                       return env_adjoint<K>(env_load_pixel(positions, colors, normals, material, radiance, occlusion,
                                                            grad, aq, H, W, rq),
                                             cam, C, unused)
                           .a;
                   },
                   acc);
        if (grad_positions) st3(grad_positions + p * 3, make_float3(acc[0], acc[1], acc[2]));
        if (grad_normals) st3(grad_normals + p * 3, make_float3(acc[3], acc[4], acc[5]));
    }
}

// where column j of a partial row goes: the camera's three elements, then the [K, 3] coefficients in index order
// (reflect_view: P = 3, no coefficients)
struct EnvParamGrads {
    float *cam, *coefficients;
};
__device__ __forceinline__ SlColumn env_column(int j, int P, int cam_pf, int coeffs_pf, const EnvParamGrads &G)
{
    SlColumn c = {nullptr, 0};
    if (j < kEnvCamSums) {
        if (G.cam) c.out = G.cam + j;
        c.stride = cam_pf ? 3 : 0;
    } else {
        if (G.coefficients) c.out = G.coefficients + (j - kEnvCamSums);
        c.stride = coeffs_pf ? P - kEnvCamSums : 0;
    }
    return c;
}

// shade_lights_reduce_kernel's shape with env_column's columns (that kernel's columns are the lights')
__global__ __launch_bounds__(kSlThreads) void shade_env_reduce_kernel(const float *__restrict__ partial, int B,
                                                                      int chunks, int P, int cam_pf, int coeffs_pf,
                                                                      EnvParamGrads G)
{
    __shared__ float wave_sums[kSlWaves];
    const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const SlColumn col = env_column(j, P, cam_pf, coeffs_pf, G);
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
