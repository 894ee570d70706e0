// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after lighting_kernels.h
// (ld3 / st3 / dot3 ..., shade_clamp, shade_clamp_grad, spec_terms, light_blocks).  Not a standalone header.  What the
// shade shares with shade_lights_kernels.h lives here: the route word's accessors (route_code, route_normal_code,
// route_normals), pixel_at, window_max, routed3 and ShadeAdjoint.  The forwards' opening, the backwards' six-sum gather
// and the diffuse and specular adjoints stay written out in each kernel: as shared functions they moved the listings
// of kernels that then measured slower, or raised a register count.
//
// The pixel-space stage of deferred shading (the reference's samples/deferred.py:85-115, as
// tests/deferred_pipeline.py::shade states it with selects): silhouette dilation of the G-buffers by a 3x3 max where
// the background shows, the validity mask, and ambient + diffuse_directional + specular_directional -- one launch
// forward and one backward instead of about thirty framework launches each way.  Pure streaming, one thread per
// pixel, no contraction (no MFMA shape); all offsets 64-bit.
//
// Dilation rule (the framework's CPU max_pool2d(x, 3, stride=1, padding=1)): the window is clipped to the frame and
// scanned in row-major order starting from its first element; the running value is replaced when v > m || isnan(v).
// So the first maximum wins ties, a NaN in the window gives NaN (the last NaN wins), an all -inf window picks its
// first element.  A window never crosses a frame of the batch.
// Route codes, 4 bits per channel: 0..8 = the winner's window position (dy + 1) * 3 + (dx + 1), 15 = not dilated
// (own value).  The general op packs C <= 8 codes from bit 0 (unused nibbles 0); the shade packs positions in bits
// 0..11, normals in bits 12..23 and `valid` in bit 31.
// Both backwards are gathers: a thread sums what is routed to its own pixel -- its own term first, then the window
// in row-major order -- so the gradients are bit-identical from run to run (no float atomics).  The 3x3 neighbourhood
// of values is read only by the lanes that need it: masked pixels forward; backward every lane reads its nine route
// words and fetches a neighbour's cotangent (the shade: recomputes its lighting adjoint) only where a code points
// back at it.

constexpr uint32_t kRouteOwn = 15u;
constexpr uint32_t kRouteValid = 0x80000000u;
constexpr int kRouteNormals = 12;  // the shade's route word: first bit of the normals' codes
// code c of a packed word (of the shade's word: position code c); normal code c of the shade's word; its normals' codes
// as a packed word of their own
__device__ __forceinline__ uint32_t route_code(uint32_t codes, int c) { return (codes >> (4 * c)) & 15u; }
__device__ __forceinline__ uint32_t route_normal_code(uint32_t r, int c) { return (r >> (kRouteNormals + 4 * c)) & 15u; }
__device__ __forceinline__ uint32_t route_normals(uint32_t r) { return r >> kRouteNormals; }

struct PixelAt {
    int64_t f0;  // first pixel of the frame
    int y, x;
};
__device__ __forceinline__ PixelAt pixel_at(int64_t p, int H, int W)
{
    const int64_t hw = (int64_t)H * W;
    const int64_t b = p / hw;
    const int r = (int)(p - b * hw);
    PixelAt a;
    a.f0 = b * hw;
    a.y = r / W;
    a.x = r - a.y * W;
    return a;
}

// the 3x3 max of channels [0, C) around pixel `at` of x [*, H, W, C]: values in m, returns the C packed codes
template <int C>
__device__ __forceinline__ uint32_t window_max(const float *__restrict__ x, PixelAt at, int H, int W, float m[C])
{
    uint32_t code[C];
    bool first = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = at.y + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = at.x + dx;
            if (xx < 0 || xx >= W) continue;
            const float *q = x + (at.f0 + (int64_t)yy * W + xx) * C;
            const uint32_t k = (uint32_t)((dy + 1) * 3 + (dx + 1));
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v = q[c];
                if (first || v > m[c] || v != v) {
                    m[c] = v;
                    code[c] = k;
                }
            }
            first = false;
        }
    }
    uint32_t packed = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) packed |= code[c] << (4 * c);
    return packed;
}

template <int C>
__device__ __forceinline__ uint32_t route_own()
{
    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) r |= kRouteOwn << (4 * c);
    return r;
}

// does any of the n codes of `codes` equal `want`?
__device__ __forceinline__ bool route_any(uint32_t codes, int n, uint32_t want)
{
    bool hit = false;
    for (int c = 0; c < n; ++c) hit = hit || route_code(codes, c) == want;
    return hit;
}

// ---- general dilation: x, out [B, H, W, C], mask [B, H, W] uint8 (NULL: any channel of x[p] is +-inf)

template <int C>
__global__ __launch_bounds__(kLightThreads) void dilate_fwd_kernel(const float *__restrict__ x,
                                                                   const uint8_t *__restrict__ mask, int H, int W,
                                                                   int64_t n, float *__restrict__ out,
                                                                   uint32_t *__restrict__ route)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float v[C];
    bool m = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        v[c] = x[p * C + c];
        m = m || isinf(v[c]);
    }
    if (mask) m = mask[p] != 0;
    uint32_t r = route_own<C>();
    if (m) r = window_max<C>(x, pixel_at(p, H, W), H, W, v);
#pragma unroll
    for (int c = 0; c < C; ++c) out[p * C + c] = v[c];
    route[p] = r;
}

template <int C>
__global__ __launch_bounds__(kLightThreads) void dilate_bwd_kernel(const float *__restrict__ grad,
                                                                   const uint32_t *__restrict__ route, int H, int W,
                                                                   int64_t n, float *__restrict__ grad_x)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    const PixelAt at = pixel_at(p, H, W);
    const uint32_t r = route[p];
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = route_code(r, c) == kRouteOwn ? grad[p * C + c] : 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = at.y + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = at.x + dx;
            if (xx < 0 || xx >= W) continue;
            const int64_t q = at.f0 + (int64_t)yy * W + xx;
            // q sees this pixel at the mirrored window position
            const uint32_t back = (uint32_t)(8 - ((dy + 1) * 3 + (dx + 1)));
            const uint32_t rq = route[q];
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (route_code(rq, c) == back) acc[c] += grad[q * C + c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) grad_x[p * C + c] = acc[c];
}

// ---- fused shade: positions, colors, normals, pixels [B, H, W, 3]

struct ShadeLights {
    const float *ambient, *ldir, *diffuse_color, *specular_color, *campos;  // device pointers to 3 floats
    float shin;
    int two;
};

// the three channels of x at pixel q as its codes route them (15: own; 0..8: the window position's); a code that
// does not name a pixel of the frame reads the own value, so no route word can address outside the frame
__device__ __forceinline__ float3 routed3(const float *__restrict__ x, PixelAt at, int H, int W, uint32_t codes)
{
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t k = route_code(codes, c);
        int yy = at.y, xx = at.x;
        if (k <= 8u) {
            const int ky = (int)(k / 3u);
            yy += ky - 1;
            xx += (int)k - 3 * ky - 1;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) {
                yy = at.y;
                xx = at.x;
            }
        }
        v[c] = x[(at.f0 + (int64_t)yy * W + xx) * 3 + c];
    }
    return make_float3(v[0], v[1], v[2]);
}

__device__ __forceinline__ bool finite3(float3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

__global__ __launch_bounds__(kLightThreads) void deferred_shade_fwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals, int H,
    int W, int64_t n, ShadeLights L, float *__restrict__ pixels, uint8_t *__restrict__ valid,
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
        const float3 col = ld3(colors + p * 3), amb = ld3(L.ambient), l = ld3(L.ldir), lcd = ld3(L.diffuse_color),
                     lcs = ld3(L.specular_color);
        const bool two = L.two != 0;
        const float cs = shade_clamp(dot3(nv, mul3(l, -1.0f)), two);
        const SpecTerms s = spec_terms(pos, nv, l, ld3(L.campos), L.shin, two);
        // (diffuse + specular) + colour * ambient, as the framework statement sums them
        px.x = (lcd.x * col.x * cs + lcs.x * col.x * s.p) + col.x * amb.x;
        px.y = (lcd.y * col.y * cs + lcs.y * col.y * s.p) + col.y * amb.y;
        px.z = (lcd.z * col.z * cs + lcs.z * col.z * s.p) + col.z * amb.z;
    }
    st3(pixels + p * 3, px);
    valid[p] = ok ? 1 : 0;
    route[p] = r | (ok ? kRouteValid : 0u);
}

// the lighting adjoints of one valid pixel with respect to its dilated position and normal and its colour
// (diffuse_bwd_kernel's and specular_bwd_kernel's arithmetic with reflectivities = colours, plus the ambient term)
struct ShadeAdjoint {
    float3 pos, nrm, col;
};
__device__ __forceinline__ ShadeAdjoint shade_adjoint(float3 pos, float3 nv, float3 col, float3 g, const ShadeLights &L)
{
    const float3 amb = ld3(L.ambient), l = ld3(L.ldir), lcd = ld3(L.diffuse_color), lcs = ld3(L.specular_color);
    const bool two = L.two != 0;
    const float3 tl = mul3(l, -1.0f);
    ShadeAdjoint a;
    // diffuse
    const float c = dot3(nv, tl), cs = shade_clamp(c, two);
    const float3 gd = make_float3(g.x * lcd.x, g.y * lcd.y, g.z * lcd.z);
    a.col = mul3(gd, cs);
    a.nrm = mul3(tl, shade_clamp_grad(c, dot3(gd, col), two));
    // specular
    const SpecTerms s = spec_terms(pos, nv, l, ld3(L.campos), L.shin, two);
    const float3 gs = make_float3(g.x * lcs.x, g.y * lcs.y, g.z * lcs.z);
    a.col = add3(a.col, mul3(gs, s.p));
    const float dpow = L.shin == 0.0f ? 0.0f : L.shin * powf(s.cs, L.shin - 1.0f);
    const float dc = shade_clamp_grad(s.c, dot3(gs, col) * dpow, two);
    const float3 du = mul3(s.r, dc), dr = mul3(s.u, dc);
    const float it = 1.0f / s.tn;
    const float3 dt = sub3(mul3(du, it), mul3(s.t, dot3(s.t, du) * it * it * it));
    a.pos = mul3(dt, -1.0f);
    a.nrm = add3(a.nrm, add3(mul3(tl, 2.0f * dot3(dr, nv)), mul3(dr, 2.0f * dot3(nv, tl))));
    // ambient
    a.col = add3(a.col, make_float3(g.x * amb.x, g.y * amb.y, g.z * amb.z));
    return a;
}

// One launch: a thread computes its own pixel's adjoint and recomputes that of each neighbour whose route points
// back at it (a few background pixels along the silhouette), rather than a [B, H, W, 6] intermediate and a second
// pass over it.
__global__ __launch_bounds__(kLightThreads) void deferred_shade_bwd_kernel(
    const float *__restrict__ positions, const float *__restrict__ colors, const float *__restrict__ normals, int H,
    int W, int64_t n, ShadeLights L, const float *__restrict__ grad, const uint32_t *__restrict__ route,
    float *__restrict__ grad_positions, float *__restrict__ grad_colors, float *__restrict__ grad_normals)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    const PixelAt at = pixel_at(p, H, W);
    const uint32_t r = route[p];
    const float3 zero = make_float3(0.0f, 0.0f, 0.0f);
    ShadeAdjoint own;
    own.pos = own.nrm = own.col = zero;
    if (r & kRouteValid)
        own = shade_adjoint(routed3(positions, at, H, W, r), routed3(normals, at, H, W, route_normals(r)),
                            ld3(colors + p * 3), ld3(grad + p * 3), L);
    if (grad_colors) st3(grad_colors + p * 3, own.col);
    if (!grad_positions && !grad_normals) return;
    float acc[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        acc[c] = route_code(r, c) == kRouteOwn ? (&own.pos.x)[c] : 0.0f;
        acc[3 + c] = route_normal_code(r, c) == kRouteOwn ? (&own.nrm.x)[c] : 0.0f;
    }
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = at.y + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = at.x + dx;
            if (xx < 0 || xx >= W) continue;
            const bool self = dy == 0 && dx == 0;
            const uint32_t back = (uint32_t)(8 - ((dy + 1) * 3 + (dx + 1)));
            PixelAt aq = at;
            aq.y = yy;
            aq.x = xx;
            const int64_t q = at.f0 + (int64_t)yy * W + xx;
            const uint32_t rq = self ? r : route[q];
            if (!(rq & kRouteValid) || !route_any(rq, 6, back)) continue;
            const ShadeAdjoint a =
                self ? own
                     : shade_adjoint(routed3(positions, aq, H, W, rq), routed3(normals, aq, H, W, route_normals(rq)),
                                     ld3(colors + q * 3), ld3(grad + q * 3), L);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (route_code(rq, c) == back) acc[c] += (&a.pos.x)[c];
                if (route_normal_code(rq, c) == back) acc[3 + c] += (&a.nrm.x)[c];
            }
        }
    }
    if (grad_positions) st3(grad_positions + p * 3, make_float3(acc[0], acc[1], acc[2]));
    if (grad_normals) st3(grad_normals + p * 3, make_float3(acc[3], acc[4], acc[5]));
}
