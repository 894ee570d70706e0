// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after shade_lights_kernels.h.
// Not a standalone header.  It shares with the other deferred kernels only inline helpers that leave their listings
// as they were: the route accessors, pixel_at, window_max, route_own, routed3 and finite3
// (deferred_kernels.h), ld3 / st3 / dot3 ... (lighting_kernels.h) and sl_wave_sum (shade_lights_kernels.h).
//
// deferred.shade_sh: the colour G-buffer lit by low-order spherical harmonics of the normal G-buffer, with gradients
// to both and to the coefficients.  normals are dilated by the 3x3 rule of deferred_kernels.h where mask is set
// (NULL: where a channel of normals[p] is +-inf); valid = the three dilated values are finite; with `normalize` the
// dilated normal n is replaced by u = n / (|n| + 1e-12) (diffuse_point's rule for its incident vector), else used
// raw.  For a valid pixel, with (x, y, z) that vector and K in {1, 4, 9} coefficients [K, 3] (bands 0, 0-1, 0-2):
//   Y0 = c0          Y1 = c1 y        Y2 = c1 z            Y3 = c1 x
//   Y4 = c2 (x y)    Y5 = c2 (y z)    Y6 = c3 (3 z^2 - 1)  Y7 = c2 (x z)    Y8 = c4 (x^2 - y^2)
//   E_c = coefficients[0,c] Y0;  E_c = E_c + coefficients[k,c] Y_k, k in index order;  pixels_c = colors_c E_c
// No clamp.  route: the normals' three codes from bit 0 (dilate's layout), valid in bit 31.
// Adjoints, g the upstream gradient: grad_colors_c = g_c E_c; gE_c = g_c colors_c; the coefficient term of (k, c) is
// gE_c Y_k; g_u = sum_k (sum_c gE_c coefficients[k,c]) grad Y_k, passed with `normalize` through
// J = I / d - h h^T |n| / d^2 (d = |n| + 1e-12, h = n / |n|, 0 at n = 0).
//
// Forward: one thread per pixel, K a template parameter, the coefficients read through a wave-uniform address.
// Backward, first kernel: a workgroup of kShThreads owns kShThreads contiguous pixels of ONE frame (grid = chunks per
// frame x min(B, 65535), the frame loop of shade_lights_bwd_kernel).  Each thread forms its pixel's adjoint; its 3 K
// coefficient terms are reduced across the wave by sl_wave_sum (a fixed tree), parked in LDS per wave, added in wave
// order by threads 0 .. 3 K - 1 and stored to workspace[frame][chunk][3 K] with plain stores.  Then grad_normals, as
// the shade's: own term first, then the window in row-major order, a neighbour's adjoint recomputed where its route
// points back (that recomputation adds nothing to a coefficient sum).  Without a coefficient gradient the kernel is
// instantiated without the sums, the LDS and the partials.
// Backward, second kernel: one workgroup per column of the partial rows; per frame, thread t adds the chunks t,
// t + 256, ... in that order, the wave butterfly and the four waves in order follow; per-frame coefficients are
// written per frame, shared ones add the frames in frame order.  Every row it reads was written by the first kernel:
// the workspace needs no clearing.  No float atomics: every gradient is bit-identical from run to run.  All offsets
// 64-bit.

constexpr int kShThreads = 256;  // the backward's workgroup, and its chunk of pixels
constexpr int kShWaves = kShThreads / 64;
constexpr int kShMaxSums = 3 * DIRT_MAX_SH_COEFFS;

constexpr float kShC0 = 0.28209479177387814f, kShC1 = 0.4886025119029199f, kShC2 = 1.0925484305920792f,
                kShC3 = 0.31539156525252005f, kShC4 = 0.5462742152960396f;

struct ShadeShArgs {
    const float *coefficients;  // [K, 3], or [B, K, 3] with per_frame
    int per_frame, normalize;
};

// the K coefficient rows of a frame (a wave-uniform address: scalar loads)
template <int K>
struct ShCoeffs {
    float3 row[K];
};
template <int K>
__device__ __forceinline__ ShCoeffs<K> sh_coeffs(const ShadeShArgs &A, int64_t frame)
{
    const float *c = A.coefficients + (A.per_frame ? frame * (3 * K) : 0);
    ShCoeffs<K> C;
#pragma unroll
    for (int k = 0; k < K; ++k) C.row[k] = ld3(c + 3 * k);
    return C;
}

// the vector the basis is evaluated at: the dilated normal, raw or over its length + eps
__device__ __forceinline__ float3 sh_direction(float3 nv, bool normalize)
{
    return normalize ? mul3(nv, 1.0f / (norm3(nv) + 1.e-12f)) : nv;
}

template <int K>
__device__ __forceinline__ void sh_basis(float3 u, float Y[K])
{
    Y[0] = kShC0;
    if constexpr (K > 1) {
        Y[1] = kShC1 * u.y;
        Y[2] = kShC1 * u.z;
        Y[3] = kShC1 * u.x;
    }
    if constexpr (K > 4) {
        Y[4] = kShC2 * (u.x * u.y);
        Y[5] = kShC2 * (u.y * u.z);
        Y[6] = kShC3 * (3.0f * (u.z * u.z) - 1.0f);
        Y[7] = kShC2 * (u.x * u.z);
        Y[8] = kShC4 * (u.x * u.x - u.y * u.y);
    }
}

template <int K>
__device__ __forceinline__ float3 sh_irradiance(const ShCoeffs<K> &C, const float Y[K])
{
    float3 E = mul3(C.row[0], Y[0]);
#pragma unroll
    for (int k = 1; k < K; ++k) E = add3(E, mul3(C.row[k], Y[k]));
    return E;
}

template <int K>
__global__ __launch_bounds__(kLightThreads) void shade_sh_fwd_kernel(
    const float *__restrict__ colors, const float *__restrict__ normals, const uint8_t *__restrict__ mask, int H, int W,
    int64_t n, ShadeShArgs A, float *__restrict__ pixels, uint8_t *__restrict__ valid, uint32_t *__restrict__ route)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float3 nv = ld3(normals + p * 3);
    const bool m = mask ? mask[p] != 0 : (isinf(nv.x) || isinf(nv.y) || isinf(nv.z));
    uint32_t r = route_own<3>();
    if (m) {
        float mn[3] = {0.0f, 0.0f, 0.0f};
        r = window_max<3>(normals, pixel_at(p, H, W), H, W, mn);
        nv = make_float3(mn[0], mn[1], mn[2]);
    }
    const bool ok = finite3(nv);
    float3 px = make_float3(0.0f, 0.0f, 0.0f);
    if (ok) {
        const int64_t frame = A.per_frame ? p / ((int64_t)H * W) : 0;
        const ShCoeffs<K> C = sh_coeffs<K>(A, frame);
        float Y[K];
        sh_basis<K>(sh_direction(nv, A.normalize != 0), Y);
        const float3 E = sh_irradiance<K>(C, Y), col = ld3(colors + p * 3);
        px = make_float3(col.x * E.x, col.y * E.y, col.z * E.z);
    }
    st3(pixels + p * 3, px);
    valid[p] = ok ? 1 : 0;
    route[p] = r | (ok ? kRouteValid : 0u);
}

struct ShAdjoint {
    float3 nrm, col;  // with respect to the dilated normal and the colour
    float3 gE;        // g * colour: the coefficient term of (k, c) is gE_c Y_k
};

// the adjoint of one valid pixel; Y receives its basis values
template <int K>
__device__ __forceinline__ ShAdjoint sh_adjoint(float3 nv, float3 col, float3 g, const ShCoeffs<K> &C, bool normalize,
                                                float Y[K])
{
    const float3 u = sh_direction(nv, normalize);
    sh_basis<K>(u, Y);
    const float3 E = sh_irradiance<K>(C, Y);
    ShAdjoint a;
    a.col = make_float3(g.x * E.x, g.y * E.y, g.z * E.z);
    a.gE = make_float3(g.x * col.x, g.y * col.y, g.z * col.z);
    float3 gu = make_float3(0.0f, 0.0f, 0.0f);
    if constexpr (K > 1) {
        float w[K];  // w_k = sum_c gE_c coefficients[k, c]
#pragma unroll
        for (int k = 1; k < K; ++k) w[k] = dot3(a.gE, C.row[k]);
        gu = make_float3(kShC1 * w[3], kShC1 * w[1], kShC1 * w[2]);
        if constexpr (K > 4) {
            gu.x += kShC2 * (u.y * w[4] + u.z * w[7]) + (2.0f * kShC4) * (u.x * w[8]);
            gu.y += kShC2 * (u.x * w[4] + u.z * w[5]) - (2.0f * kShC4) * (u.y * w[8]);
            gu.z += kShC2 * (u.y * w[5] + u.x * w[7]) + (6.0f * kShC3) * (u.z * w[6]);
        }
    }
    if (normalize) {
        // u = n / (|n| + eps): dn = gu / (|n| + eps) - n (n . gu) / (|n| (|n| + eps)^2), the second term 0 at n = 0
        const float len = norm3(nv), d = len + 1.e-12f;
        float3 dn = mul3(gu, 1.0f / d);
        if (len > 0.0f) dn = sub3(dn, mul3(nv, dot3(nv, gu) / (len * d * d)));
        gu = dn;
    }
    a.nrm = gu;
    return a;
}

template <int K, bool kParams>
__global__ __launch_bounds__(kShThreads) void shade_sh_bwd_kernel(
    const float *__restrict__ colors, const float *__restrict__ normals, int B, int H, int W, ShadeShArgs A,
    const float *__restrict__ grad, const uint32_t *__restrict__ route, float *__restrict__ grad_colors,
    float *__restrict__ grad_normals, float *__restrict__ partial)
{
    __shared__ float wave_sums[kParams ? kShWaves : 1][kParams ? kShMaxSums : 1];
    constexpr int P = 3 * K;
    const int64_t hw = (int64_t)H * W;
    const int chunk = blockIdx.x, chunks = gridDim.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool normalize = A.normalize != 0;
    const float3 zero = make_float3(0.0f, 0.0f, 0.0f);
    const int64_t in_frame = (int64_t)chunk * kShThreads + tid;
    const bool inside = in_frame < hw;
    // (a grid's second dimension holds fewer frames than a batch may have)
    for (int64_t frame = blockIdx.y; frame < B; frame += gridDim.y) {
        const ShCoeffs<K> C = sh_coeffs<K>(A, frame);
        PixelAt at;
        at.f0 = frame * hw;
        at.y = inside ? (int)(in_frame / W) : 0;
        at.x = inside ? (int)(in_frame - (int64_t)at.y * W) : 0;
        const int64_t p = at.f0 + in_frame;
        const uint32_t r = inside ? route[p] : 0u;
        const bool ok = (r & kRouteValid) != 0;
        ShAdjoint own;
        own.nrm = own.col = own.gE = zero;
        float Y[K];
#pragma unroll
        for (int k = 0; k < K; ++k) Y[k] = 0.0f;
        if (ok)
            own = sh_adjoint<K>(routed3(normals, at, H, W, r), ld3(colors + p * 3), ld3(grad + p * 3), C, normalize,
                                Y);
        if (kParams) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float s = sl_wave_sum(ok ? (&own.gE.x)[c] * Y[k] : 0.0f);
                    if (lane == 0) wave_sums[wave][3 * k + c] = s;
                }
            }
            __syncthreads();
            if (tid < P) {
                float s = wave_sums[0][tid];
#pragma unroll
                for (int w = 1; w < kShWaves; ++w) s += wave_sums[w][tid];
                partial[(frame * chunks + chunk) * P + tid] = s;
            }
            __syncthreads();  // (the next frame of this workgroup writes wave_sums again)
        }
        if (!inside) continue;
        if (grad_colors) st3(grad_colors + p * 3, own.col);
        if (!grad_normals) continue;
        // the normals' gradient: own term first, then the window in row-major order
        float acc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = route_code(r, c) == kRouteOwn ? (&own.nrm.x)[c] : 0.0f;
#pragma unroll 1
        for (int w = 0; w < 9; ++w) {
            const int dy = w / 3 - 1, dx = w - 3 * (w / 3) - 1;
            const int yy = at.y + dy, xx = at.x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const bool self = w == 4;
            const uint32_t back = (uint32_t)(8 - w);  // the neighbour sees this pixel at the mirrored position
            const int64_t q = at.f0 + (int64_t)yy * W + xx;
            const uint32_t rq = self ? r : route[q];
            const bool back0 = route_code(rq, 0) == back, back1 = route_code(rq, 1) == back,
                       back2 = route_code(rq, 2) == back;
            if (!(rq & kRouteValid) || !(back0 || back1 || back2)) continue;
            float3 a = own.nrm;
            if (!self) {
                PixelAt aq = at;
                aq.y = yy;
                aq.x = xx;
                float unused[K];
                a = sh_adjoint<K>(routed3(normals, aq, H, W, rq), ld3(colors + q * 3), ld3(grad + q * 3), C, normalize,
                                  unused)
                        .nrm;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (route_code(rq, c) == back) acc[c] += (&a.x)[c];
        }
        st3(grad_normals + p * 3, make_float3(acc[0], acc[1], acc[2]));
    }
}

// column j of the partial rows is element j of a frame's [K, 3] gradient; per_frame: one such gradient per frame
__global__ __launch_bounds__(kShThreads) void shade_sh_reduce_kernel(const float *__restrict__ partial, int B,
                                                                     int chunks, int P, int per_frame,
                                                                     float *__restrict__ grad_coefficients)
{
    __shared__ float wave_sums[kShWaves];
    const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float total = 0.0f;
    for (int64_t frame = 0; frame < B; ++frame) {
        float s = 0.0f;
        for (int64_t c = tid; c < chunks; c += kShThreads) s += partial[(frame * chunks + c) * P + j];
        s = sl_wave_sum(s);
        if (lane == 0) wave_sums[wave] = s;
        __syncthreads();
        float f = wave_sums[0];
#pragma unroll
        for (int w = 1; w < kShWaves; ++w) f += wave_sums[w];
        __syncthreads();
        if (per_frame) {
            if (tid == 0) grad_coefficients[frame * P + j] = f;
        } else {
            total = frame == 0 ? f : total + f;
        }
    }
    if (!per_frame && tid == 0) grad_coefficients[j] = total;
}
