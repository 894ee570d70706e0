// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after texture_kernels.h, whose
// per-level rules (tex_axis, tex_bilinear, tex_grad_uv, tex_add_taps, tex_box_reduce, tex_flush_add) it calls with a
// cube face as the level.  Not a standalone header.
//
// Cube-map lookup: bilinear sampling of a cube map [Cf, 6, S, S, C] (Cf = 1: shared by the frames, Cf = B: one per
// frame; faces +x, -x, +y, -y, +z, -z, each laid out as a texture of texture_kernels.h) at a direction G-buffer
// [B, H, W, 3], and its gradients.  The directions need not be unit length.
//
// Rule, float32, every line one IEEE operation (the build has -ffp-contract=off); (x, y, z) the direction:
//   major axis: x if |x| >= |y| && |x| >= |z|, else y if |y| >= |z|, else z;  ma = that component
//   the face is the negative one exactly when ma < 0 (-0.0 takes the positive face); the OpenGL table:
//     +x: sc = -z, tc = -y    -x: sc = +z, tc = -y    +y: sc = +x, tc = +z
//     -y: sc = +x, tc = -z    +z: sc = +x, tc = -y    -z: sc = -x, tc = -y
//   m = |ma|;  su = sc / m;  sv = tc / m;  u = su + 1;  u = u * 0.5;  v = sv + 1;  v = v * 0.5
// |sc|, |tc| <= m, so u and v lie in [0, 1]; the face's texels are filtered by tex_axis(u, S, clamp),
// tex_axis(v, S, clamp) and tex_bilinear: filtering clamps to the face's edge, there is none across face seams.
// A pixel is sampled where the mask is nonzero (mask NULL: everywhere) and the direction's three values are finite and
// not all zero; the others give exactly 0, carry no gradient and never form an address.
//
// Backward, one launch, with g = grad_texels[p, :] at sampled pixels:
//   (gu, gv) = tex_grad_uv on the face (pass is always true: u, v in [0, 1])
//   hu = 0.5 * gu;  hv = 0.5 * gv;  g_sc = hu / m;  g_tc = hv / m
//   t = hu * su;  t2 = hv * sv;  t = t + t2;  g_m = t / m;  g_m = -g_m;  g_ma = ma < 0 ? -g_m : g_m
// written to x, y, z through the table's signs: a gather in a fixed order, bit-identical from run to run.  The
// cube map's gradient is tex_add_taps' scatter into the selected face of the pixel's frame, with float atomics.  A
// 256-thread workgroup owns a 16 x 16 screen tile as texture_sample_bwd_kernel does; when every sampled lane of the
// tile lies on one face and the box of their taps holds at most kCubePatchTexels texels it sums the tile's terms in
// an LDS patch and flushes that, otherwise (a tile on a seam or a cube corner, minification, scattered directions)
// it adds straight to memory.

#ifndef DIRT_CUBEMAP_PATCH
#define DIRT_CUBEMAP_PATCH DIRT_TEXTURE_PATCH  // texels of the LDS patch; 0 builds the direct-atomics-only kernel (A/B)
#endif
constexpr int kCubePatchTexels = DIRT_CUBEMAP_PATCH;

// the face of a sampled direction and its coordinates on it
struct CubeCoord {
    int face;
    float ma, m, su, sv, u, v;
};

__device__ __forceinline__ bool cube_sampled(const float *__restrict__ directions, const uint8_t *__restrict__ mask,
                                             int64_t p, float *x, float *y, float *z)
{
    *x = directions[p * 3];
    *y = directions[p * 3 + 1];
    *z = directions[p * 3 + 2];
    const bool usable = isfinite(*x) && isfinite(*y) && isfinite(*z) && !(*x == 0.0f && *y == 0.0f && *z == 0.0f);
    return usable && (!mask || mask[p] != 0);
}

__device__ __forceinline__ CubeCoord cube_coord(float x, float y, float z)
{
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    CubeCoord r;
    float sc, tc;
    if (ax >= ay && ax >= az) {
        r.ma = x;
        const bool neg = x < 0.0f;
        r.face = neg ? 1 : 0;
        sc = neg ? z : -z;
        tc = -y;
    } else if (ay >= az) {
        r.ma = y;
        const bool neg = y < 0.0f;
        r.face = neg ? 3 : 2;
        sc = x;
        tc = neg ? -z : z;
    } else {
        r.ma = z;
        const bool neg = z < 0.0f;
        r.face = neg ? 5 : 4;
        sc = neg ? -x : x;
        tc = -y;
    }
    r.m = fabsf(r.ma);
    r.su = sc / r.m;
    r.sv = tc / r.m;
    float u = r.su + 1.0f;
    r.u = u * 0.5f;
    float v = r.sv + 1.0f;
    r.v = v * 0.5f;
    return r;
}

// the direction's gradient from the face coordinates' (gu, gv), through the table's signs
__device__ __forceinline__ void cube_grad_direction(const CubeCoord &cc, float gu, float gv, float *gx, float *gy,
                                                    float *gz)
{
    const float hu = 0.5f * gu, hv = 0.5f * gv;
    const float g_sc = hu / cc.m, g_tc = hv / cc.m;
    float t = hu * cc.su;
    const float t2 = hv * cc.sv;
    t = t + t2;
    float g_m = t / cc.m;
    g_m = -g_m;
    const float g_ma = cc.ma < 0.0f ? -g_m : g_m;
    switch (cc.face) {
    case 0: *gx = g_ma, *gy = -g_tc, *gz = -g_sc; break;
    case 1: *gx = g_ma, *gy = -g_tc, *gz = g_sc; break;
    case 2: *gx = g_sc, *gy = g_ma, *gz = g_tc; break;
    case 3: *gx = g_sc, *gy = g_ma, *gz = -g_tc; break;
    case 4: *gx = g_sc, *gy = -g_tc, *gz = g_ma; break;
    default: *gx = -g_sc, *gy = -g_tc, *gz = g_ma; break;
    }
}

template <int C>
__global__ __launch_bounds__(kLightThreads) void cubemap_sample_fwd_kernel(
    const float *__restrict__ cubemap, int64_t frame_stride, int S, const float *__restrict__ directions,
    const uint8_t *__restrict__ mask, int64_t hw, int64_t n, float *__restrict__ texels, uint8_t *__restrict__ valid)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float x, y, z;
    const bool ok = cube_sampled(directions, mask, p, &x, &y, &z);
    float out[C];
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = 0.0f;
    if (ok) {
        const CubeCoord cc = cube_coord(x, y, z);
        const TexAxis ax = tex_axis(cc.u, S, DIRT_TEXTURE_CLAMP), ay = tex_axis(cc.v, S, DIRT_TEXTURE_CLAMP);
        const int64_t face_base = (p / hw) * frame_stride + (int64_t)cc.face * S * S * C;
        tex_bilinear<C>(cubemap + face_base, S, ax, ay, out);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) texels[p * C + c] = out[c];
    valid[p] = ok ? 1 : 0;
}

// One workgroup per 16 x 16 screen tile of one frame (blockIdx.x = (frame * tiles_y + tile_y) * tiles_x + tile_x).
template <int C>
__global__ __launch_bounds__(kLightThreads) void cubemap_sample_bwd_kernel(
    const float *__restrict__ cubemap, int64_t frame_stride, int S, const float *__restrict__ directions,
    const uint8_t *__restrict__ mask, int H, int W, int tiles_x, int tiles_y, const float *__restrict__ grad,
    float *__restrict__ grad_cubemap, float *__restrict__ grad_directions)
{
    __shared__ float s_patch[(kCubePatchTexels > 0 ? kCubePatchTexels : 1) * C];
    __shared__ int s_box[6];  // tex_box_reduce's four words, then min face, -(max face)

    const int tx = (int)(blockIdx.x % (unsigned)tiles_x);
    const int64_t rest = blockIdx.x / (unsigned)tiles_x;
    const int ty = (int)(rest % tiles_y);
    const int64_t frame = rest / tiles_y;
    const int y = ty * kTexTile + (int)(threadIdx.x / kTexTile), x = tx * kTexTile + (int)(threadIdx.x % kTexTile);
    const bool inside = y < H && x < W;
    const int64_t p = (frame * H + (inside ? y : 0)) * W + (inside ? x : 0);

    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    const bool ok = inside && cube_sampled(directions, mask, p, &dx, &dy, &dz);
    CubeCoord cc = {0, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    TexAxis ax = kTexNoAxis, ay = ax;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = 0.0f;
    if (ok) {
        cc = cube_coord(dx, dy, dz);
        ax = tex_axis(cc.u, S, DIRT_TEXTURE_CLAMP);
        ay = tex_axis(cc.v, S, DIRT_TEXTURE_CLAMP);
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = grad[p * C + c];
    }
    const int64_t face_floats = (int64_t)S * S * C, fbase = frame * frame_stride;

    if (grad_directions && inside) {
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (ok) {
            float gu, gv;
            tex_grad_uv<C>(cubemap + fbase + cc.face * face_floats, S, S, ax, ay, g, &gu, &gv);
            cube_grad_direction(cc, gu, gv, &gx, &gy, &gz);
        }
        grad_directions[p * 3] = gx;
        grad_directions[p * 3 + 1] = gy;
        grad_directions[p * 3 + 2] = gz;
    }
    if (!grad_cubemap) return;  // (uniform)

    if (kCubePatchTexels > 0) {
        if (threadIdx.x < 6) s_box[threadIdx.x] = kTexBoxEmpty;
        __syncthreads();
        tex_box_reduce(ok, ax, ay, s_box);
        const int lo_f = wave_min(ok ? cc.face : kTexBoxEmpty), hi_f = wave_min(ok ? -cc.face : kTexBoxEmpty);
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&s_box[4], lo_f);
            atomicMin(&s_box[5], hi_f);
        }
        __syncthreads();
        const int r0 = s_box[0], c0 = s_box[2], face = s_box[4];
        if (r0 == kTexBoxEmpty) return;  // no sampled pixel in the tile (uniform)
        const int bh = -s_box[1] - r0 + 1, bw = -s_box[3] - c0 + 1;
        if (face == -s_box[5] && (int64_t)bh * bw <= kCubePatchTexels) {  // (uniform: all from LDS)
            const int ne = bh * bw * C;
            for (int e = threadIdx.x; e < ne; e += kLightThreads) s_patch[e] = 0.0f;
            __syncthreads();
            if (ok) tex_add_taps<C>(s_patch, r0, c0, bw, ax, ay, g, 1.0f);
            __syncthreads();
            // (tex_flush_patch's loop, restated: a third caller of it reorders two instructions of that loop in
            // texture_sample_bwd_kernel, and the existing kernels' code stays as it is)
            float *gf = grad_cubemap + fbase + face * face_floats;
            for (int e = threadIdx.x; e < ne; e += kLightThreads) {
                const float s = s_patch[e];
                if (s != 0.0f) tex_flush_add<C>(s, e, r0, c0, bw, gf, S);
            }
            return;
        }
    }
    if (ok) tex_add_taps<C>(grad_cubemap + fbase + cc.face * face_floats, 0, 0, S, ax, ay, g, 1.0f);
}
