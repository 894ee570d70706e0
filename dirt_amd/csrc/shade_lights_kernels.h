// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after deferred_kernels.h.  Not a
// standalone header.  What it shares with the shade lives there (the route accessors, pixel_at, window_max, routed3,
// ShadeAdjoint) and in lighting_kernels.h (spec_terms, shade_clamp); the forward's opening, the gather and the
// per-light adjoints are written out here as in the shade (DESIGN.md 7k has why).  It is not the shade with N = 1: the
// shade's adjoint sums start at x, these at 0 + x (the sign of a zero), and the parameters are loaded differently.
//
// deferred.shade_lights: deferred_kernels.h's shade with up to DIRT_MAX_LIGHTS lights, each directional or a point
// light, and with gradients to the lights, the camera, the ambient colour and the shininess.  Dilation, `valid` and
// the route word are the shade's.  For a valid pixel, the lights in index order:
//   acc = (d_0 + s_0);  acc = acc + (d_i + s_i) ...;  pixels = acc + colors * ambient
// directional light (its row l is the direction, used raw): d = dc * colour * clamp(n . (-l)),
//   s = sc * colour * clamp((t / |t| + eps) . r)^k with r = l + 2 (n . (-l)) n, t = cam - p  (spec_terms)
// point light (its row is the position): u = (p - light) / (|p - light| + eps), d = dc * colour * clamp(n . u),
//   s = the directional s with u in place of l; the adjoint of u flows into p and, negated, into the light's position.
//
// Forward: one thread per pixel, a loop over the lights, a branch per light on the mask bit (uniform over the launch).
// Backward, first kernel: a workgroup of kSlThreads owns a chunk of kSlChunk contiguous pixels of ONE frame (grid =
// chunks per frame x frames), each thread kSlPixelsPerThread pixels strided by the block size.  The lights are the
// outer loop: per light a thread adds the light's adjoint into its pixels' (position, normal, colour) adjoints and
// sums the light's nine parameter terms over its pixels; those nine are reduced across the wave by a __shfl_xor
// butterfly (a fixed tree) and parked in LDS per wave -- no thread holds 9 N accumulators.  After the last light the
// seven light-independent sums (ambient 3, camera 3, shininess 1) follow, one barrier, and threads 0 .. P-1 add the
// four waves' values in wave order and store the chunk's P = 7 + 9 N partial sums to workspace[frame][chunk][P] with
// plain stores.  Then the G-buffer gradients, as the shade's: own adjoint first, then the window in row-major order,
// a neighbour's adjoint recomputed where its route points back (that recomputation adds nothing to a parameter: a
// pixel's parameter terms are counted once, by the thread that owns it).
// Backward, second kernel (launched after the first on the same stream; the kernel boundary is the hand-off): one
// workgroup per column of the partial rows.  Per frame, thread t adds the chunks t, t + 256, ... in that order, the
// wave butterfly and the four waves in order follow; a per-frame parameter is written per frame, a shared one adds
// the frames in frame order.  Every row the second kernel reads was written by the first: the workspace needs no
// clearing.  No float atomics anywhere: every gradient is bit-identical from run to run.
// With no parameter gradient requested the first kernel is instantiated without the sums, the partials and the LDS,
// and the second is not launched.  All offsets 64-bit.

constexpr int kSlThreads = 256;
// the tuning knob of the backward: pixels per thread, and with it the chunk (DESIGN.md 7j records what was tried;
// 4, 2 and 1 were measured, 1 ships; `make variant DEFS=-DDIRT_SL_PIXELS_PER_THREAD=2` builds another)
#ifndef DIRT_SL_PIXELS_PER_THREAD
#define DIRT_SL_PIXELS_PER_THREAD 1
#endif
constexpr int kSlPixelsPerThread = DIRT_SL_PIXELS_PER_THREAD;
constexpr int kSlChunk = kSlThreads * kSlPixelsPerThread;  // 256 pixels per workgroup
constexpr int kSlWaves = kSlThreads / 64;
constexpr int kSlFixedSums = 7;      // ambient 3, camera 3, shininess 1
constexpr int kSlSumsPerLight = 9;   // light vector 3, diffuse colour 3, specular colour 3
constexpr int kSlMaxSums = kSlFixedSums + kSlSumsPerLight * DIRT_MAX_LIGHTS;

struct ShadeLightsArgs {
    const float *ambient;                // 3 floats, or NULL (zero)
    const float *lvec, *dcol, *scol;     // [N, 3], or [B, N, 3] with lights_pf
    const float *cam;                    // [3], or [B, 3] with cam_pf
    const float *shin_ptr;               // one float, or NULL (shin)
    float shin;
    int n;
    uint32_t point_mask;
    int lights_pf, cam_pf, two;
};

struct SlLight {
    float3 v, dc, sc;
    bool point;
};
__device__ __forceinline__ SlLight sl_light(const ShadeLightsArgs &A, int64_t frame, int i)
{
    const int64_t o = ((A.lights_pf ? frame * A.n : 0) + i) * 3;
    SlLight L;
    L.v = ld3(A.lvec + o);
    L.dc = ld3(A.dcol + o);
    L.sc = ld3(A.scol + o);
    L.point = ((A.point_mask >> i) & 1u) != 0;
    return L;
}
__device__ __forceinline__ float3 sl_camera(const ShadeLightsArgs &A, int64_t frame)
{
    return A.n > 0 ? ld3(A.cam + (A.cam_pf ? frame * 3 : 0)) : make_float3(0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ float3 sl_ambient(const ShadeLightsArgs &A)
{
    return A.ambient ? ld3(A.ambient) : make_float3(0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ float sl_shininess(const ShadeLightsArgs &A) { return A.shin_ptr ? *A.shin_ptr : A.shin; }
__device__ __forceinline__ float3 mul33(float3 a, float3 b) { return make_float3(a.x * b.x, a.y * b.y, a.z * b.z); }

__global__ __launch_bounds__(kLightThreads) void shade_lights_fwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals, int H,
    int W, int64_t n, ShadeLightsArgs A, float *__restrict__ pixels, uint8_t *__restrict__ valid,
    uint32_t *__restrict__ route)
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
        const float3 col = ld3(colors + p * 3), amb = sl_ambient(A), cam = sl_camera(A, frame);
        const float shin = sl_shininess(A);
        const bool two = A.two != 0;
        float3 acc = make_float3(0.0f, 0.0f, 0.0f);
        for (int i = 0; i < A.n; ++i) {
            const SlLight L = sl_light(A, frame, i);
            float3 l = L.v, towards = mul3(L.v, -1.0f);  // the normal is dotted with -l, or with u
            if (L.point) {
                const float3 rel = sub3(pos, L.v);
                l = towards = mul3(rel, 1.0f / (norm3(rel) + 1.e-12f));
            }
            const float cs = shade_clamp(dot3(nv, towards), two);
            const SpecTerms s = spec_terms(pos, nv, l, cam, shin, two);
            const float3 term = make_float3(L.dc.x * col.x * cs + L.sc.x * col.x * s.p,
                                            L.dc.y * col.y * cs + L.sc.y * col.y * s.p,
                                            L.dc.z * col.z * cs + L.sc.z * col.z * s.p);
            acc = i == 0 ? term : add3(acc, term);
        }
        px = add3(acc, mul33(col, amb));
    }
    st3(pixels + p * 3, px);
    valid[p] = ok ? 1 : 0;
    route[p] = r | (ok ? kRouteValid : 0u);
}

struct SlPixel {
    float3 pos, nv, col, g;  // dilated position and normal, colour, upstream gradient
};
// the per-light parameter terms of one pixel and the light-independent ones it shares with the other lights
struct SlParamTerms {
    float light[kSlSumsPerLight];
    float3 cam;
    float shin;
};

// one light's adjoint of one valid pixel, added into `a` (diffuse_bwd_kernel's / diffuse_point_bwd_kernel's and
// specular_bwd_kernel's arithmetic with reflectivities = colours); with kParams its parameter terms added into `t`
template <bool kParams>
__device__ __forceinline__ void sl_light_adjoint(const SlPixel &x, const SlLight &L, float3 cam, float shin, bool two,
                                                 ShadeAdjoint &a, SlParamTerms &t)
{
    float3 l = L.v, rel = make_float3(0.0f, 0.0f, 0.0f);
    float m = 0.0f, dm = 1.0f;
    if (L.point) {
        rel = sub3(x.pos, L.v);
        m = norm3(rel);
        dm = m + 1.e-12f;
        l = mul3(rel, 1.0f / dm);
    }
    const float3 tl = mul3(l, -1.0f);
    const float3 towards = L.point ? l : tl;
    // diffuse
    const float c = dot3(x.nv, towards), cs = shade_clamp(c, two);
    const float3 gd = mul33(x.g, L.dc);
    a.col = add3(a.col, mul3(gd, cs));
    const float gc = shade_clamp_grad(c, dot3(gd, x.col), two);
    a.nrm = add3(a.nrm, mul3(towards, gc));
    float3 dl = mul3(x.nv, L.point ? gc : -gc);  // the adjoint of l (of u for a point light)
    // specular
    const SpecTerms s = spec_terms(x.pos, x.nv, l, cam, shin, two);
    const float3 gs = mul33(x.g, L.sc);
    a.col = add3(a.col, mul3(gs, s.p));
    const float gp = dot3(gs, x.col);
    const float dpow = shin == 0.0f ? 0.0f : shin * powf(s.cs, shin - 1.0f);
    const float dc = shade_clamp_grad(s.c, gp * dpow, two);
    const float3 du = mul3(s.r, dc), dr = mul3(s.u, dc);
    const float it = 1.0f / s.tn;
    const float3 dt = sub3(mul3(du, it), mul3(s.t, dot3(s.t, du) * it * it * it));
    a.pos = add3(a.pos, mul3(dt, -1.0f));
    a.nrm = add3(a.nrm, add3(mul3(tl, 2.0f * dot3(dr, x.nv)), mul3(dr, 2.0f * dot3(x.nv, tl))));
    // r = l + 2 (n . (-l)) n: dl = dr - 2 (n . dr) n
    dl = add3(dl, sub3(dr, mul3(x.nv, 2.0f * dot3(x.nv, dr))));
    if (L.point) {
        // u = rel / (|rel| + eps): d rel = du / (|rel| + eps) - rel (rel . du) / (|rel| (|rel| + eps)^2);
        // the position receives it, the light's position its negative
        float3 dd = mul3(dl, 1.0f / dm);
        if (m > 0.0f) dd = sub3(dd, mul3(rel, dot3(rel, dl) / (m * dm * dm)));
        a.pos = add3(a.pos, dd);
        dl = mul3(dd, -1.0f);
    }
    if (kParams) {
        const float3 gcol = mul33(x.g, x.col);
        t.light[0] += dl.x;
        t.light[1] += dl.y;
        t.light[2] += dl.z;
        t.light[3] += gcol.x * cs;
        t.light[4] += gcol.y * cs;
        t.light[5] += gcol.z * cs;
        t.light[6] += gcol.x * s.p;
        t.light[7] += gcol.y * s.p;
        t.light[8] += gcol.z * s.p;
        t.cam = add3(t.cam, dt);
        // d cs^k / dk = cs^k ln cs, 0 at cs = 0
        t.shin += gp * (s.cs > 0.0f ? s.p * logf(s.cs) : s.cs == 0.0f ? 0.0f : __builtin_nanf(""));
    }
}

// the whole adjoint of a valid pixel that another thread owns: every light in index order, then the ambient term
__device__ __forceinline__ ShadeAdjoint sl_adjoint(const SlPixel &x, const ShadeLightsArgs &A, int64_t frame,
                                                   float3 cam, float3 amb, float shin)
{
    ShadeAdjoint a;
    a.pos = a.nrm = a.col = make_float3(0.0f, 0.0f, 0.0f);
    SlParamTerms unused;
    for (int i = 0; i < A.n; ++i)
        sl_light_adjoint<false>(x, sl_light(A, frame, i), cam, shin, A.two != 0, a, unused);
    a.col = add3(a.col, mul33(x.g, amb));
    return a;
}

__device__ __forceinline__ SlPixel sl_load_pixel(const float *__restrict__ positions, const float *__restrict__ colors,
                                                 const float *__restrict__ normals, const float *__restrict__ grad,
                                                 PixelAt at, int H, int W, uint32_t r)
{
    const int64_t q = at.f0 + (int64_t)at.y * W + at.x;
    SlPixel x;
    x.pos = routed3(positions, at, H, W, r);
    x.nv = routed3(normals, at, H, W, route_normals(r));
    x.col = ld3(colors + q * 3);
    x.g = ld3(grad + q * 3);
    return x;
}

// the sum over the wave, in every lane: a butterfly, the same tree whatever the values
__device__ __forceinline__ float sl_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool kParams>
__global__ __launch_bounds__(kSlThreads) void shade_lights_bwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals, int B,
    int H, int W, ShadeLightsArgs A, const float *__restrict__ grad, const uint32_t *__restrict__ route,
    float *__restrict__ grad_positions, float *__restrict__ grad_colors, float *__restrict__ grad_normals,
    float *__restrict__ partial)
{
    __shared__ float wave_sums[kParams ? kSlWaves : 1][kParams ? kSlMaxSums : 1];
    const int64_t hw = (int64_t)H * W;
    const int chunk = blockIdx.x, chunks = gridDim.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = kSlFixedSums + kSlSumsPerLight * A.n;
    const float3 zero = make_float3(0.0f, 0.0f, 0.0f);
    const float3 amb = sl_ambient(A);
    const float shin = sl_shininess(A);
    const bool two = A.two != 0;
    // (a grid's second dimension holds fewer frames than a batch may have)
    for (int64_t frame = blockIdx.y; frame < B; frame += gridDim.y) {
        const float3 cam = sl_camera(A, frame);
        SlPixel x[kSlPixelsPerThread];
        ShadeAdjoint own[kSlPixelsPerThread];
        PixelAt at[kSlPixelsPerThread];
        uint32_t r[kSlPixelsPerThread];
        bool inside[kSlPixelsPerThread], ok[kSlPixelsPerThread];
#pragma unroll
        for (int k = 0; k < kSlPixelsPerThread; ++k) {
            const int64_t in_frame = (int64_t)chunk * kSlChunk + k * kSlThreads + tid;
            inside[k] = in_frame < hw;
            at[k].f0 = frame * hw;
            at[k].y = inside[k] ? (int)(in_frame / W) : 0;
            at[k].x = inside[k] ? (int)(in_frame - (int64_t)at[k].y * W) : 0;
            r[k] = inside[k] ? route[at[k].f0 + in_frame] : 0u;
            ok[k] = (r[k] & kRouteValid) != 0;
            own[k].pos = own[k].nrm = own[k].col = zero;
            x[k].pos = x[k].nv = x[k].col = x[k].g = zero;
            if (ok[k]) x[k] = sl_load_pixel(positions, colors, normals, grad, at[k], H, W, r[k]);
        }
        SlParamTerms t;
        t.cam = zero;
        t.shin = 0.0f;
        for (int i = 0; i < A.n; ++i) {
            const SlLight L = sl_light(A, frame, i);
#pragma unroll
            for (int j = 0; j < kSlSumsPerLight; ++j) t.light[j] = 0.0f;
#pragma unroll
            for (int k = 0; k < kSlPixelsPerThread; ++k)
                if (ok[k]) sl_light_adjoint<kParams>(x[k], L, cam, shin, two, own[k], t);
            if (kParams) {
#pragma unroll
                for (int j = 0; j < kSlSumsPerLight; ++j) {
                    const float s = sl_wave_sum(t.light[j]);
                    if (lane == 0) wave_sums[wave][kSlFixedSums + kSlSumsPerLight * i + j] = s;
                }
            }
        }
        float3 gamb = zero;
#pragma unroll
        for (int k = 0; k < kSlPixelsPerThread; ++k) {
            if (!ok[k]) continue;
            own[k].col = add3(own[k].col, mul33(x[k].g, amb));
            if (kParams) gamb = add3(gamb, mul33(x[k].g, x[k].col));
        }
        if (kParams) {
            const float fixed[kSlFixedSums] = {gamb.x, gamb.y, gamb.z, t.cam.x, t.cam.y, t.cam.z, t.shin};
#pragma unroll
            for (int j = 0; j < kSlFixedSums; ++j) {
                const float s = sl_wave_sum(fixed[j]);
                if (lane == 0) wave_sums[wave][j] = s;
            }
            __syncthreads();
            if (tid < P) {
                float s = wave_sums[0][tid];
#pragma unroll
                for (int w = 1; w < kSlWaves; ++w) s += wave_sums[w][tid];
                partial[(frame * chunks + chunk) * P + tid] = s;
            }
            __syncthreads();  // (the next frame of this workgroup writes wave_sums again)
        }
        // the G-buffer gradients: own term first, then the window in row-major order
#pragma unroll
        for (int k = 0; k < kSlPixelsPerThread; ++k) {
            if (!inside[k]) continue;
            const int64_t p = at[k].f0 + (int64_t)at[k].y * W + at[k].x;
            if (grad_colors) st3(grad_colors + p * 3, own[k].col);
            if (!grad_positions && !grad_normals) continue;
            float acc[6];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] = route_code(r[k], c) == kRouteOwn ? (&own[k].pos.x)[c] : 0.0f;
                acc[3 + c] = route_normal_code(r[k], c) == kRouteOwn ? (&own[k].nrm.x)[c] : 0.0f;
            }
#pragma unroll 1
            for (int w = 0; w < 9; ++w) {
                const int dy = w / 3 - 1, dx = w - 3 * (w / 3) - 1;
                const int yy = at[k].y + dy, xx = at[k].x + dx;
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                const bool self = w == 4;
                const uint32_t back = (uint32_t)(8 - w);  // the neighbour sees this pixel at the mirrored position
                PixelAt aq = at[k];
                aq.y = yy;
                aq.x = xx;
                const uint32_t rq = self ? r[k] : route[at[k].f0 + (int64_t)yy * W + xx];
                if (!(rq & kRouteValid) || !route_any(rq, 6, back)) continue;
                ShadeAdjoint a = own[k];
                if (!self)
                    a = sl_adjoint(sl_load_pixel(positions, colors, normals, grad, aq, H, W, rq), A, frame, cam, amb,
                                   shin);
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
}

// where column j of a partial row goes: the output element of frame 0, and the distance in floats from one frame's
// element to the next (0: the parameter is shared by the frames)
struct SlColumn {
    float *out;
    int64_t stride;
};
struct SlParamGrads {
    float *ambient, *lvec, *dcol, *scol, *cam, *shin;
};
__device__ __forceinline__ SlColumn sl_column(int j, int n_lights, int lights_pf, int cam_pf, const SlParamGrads &G)
{
    SlColumn c = {nullptr, 0};
    if (j < 3) {
        if (G.ambient) c.out = G.ambient + j;
    } else if (j < 6) {
        if (G.cam) c.out = G.cam + (j - 3);
        c.stride = cam_pf ? 3 : 0;
    } else if (j == 6) {
        c.out = G.shin;
    } else {
        const int i = (j - kSlFixedSums) / kSlSumsPerLight, e = (j - kSlFixedSums) - i * kSlSumsPerLight;
        float *base = e < 3 ? G.lvec : e < 6 ? G.dcol : G.scol;
        if (base) c.out = base + i * 3 + (e % 3);
        c.stride = lights_pf ? (int64_t)n_lights * 3 : 0;
    }
    return c;
}

__global__ __launch_bounds__(kSlThreads) void shade_lights_reduce_kernel(const float *__restrict__ partial, int B,
                                                                         int chunks, int n_lights, int lights_pf,
                                                                         int cam_pf, SlParamGrads G)
{
    __shared__ float wave_sums[kSlWaves];
    const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = kSlFixedSums + kSlSumsPerLight * n_lights;
    const SlColumn col = sl_column(j, n_lights, lights_pf, cam_pf, G);
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
