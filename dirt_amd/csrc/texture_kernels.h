// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after deferred_kernels.h
// (kLightThreads, light_blocks).  Not a standalone header.  It holds every rule of one texture level, each once, as
// tex_* device functions that texture_mip_kernels.h calls per level too: tex_axis, tex_sampled, tex_bilinear (the
// value), tex_grad_uv, tex_add_taps (the scatter, to memory or an LDS box), tex_box_reduce, tex_flush_add / _patch.
//
// Deferred texturing: bilinear sampling of a texture [Tf, Th, Tw, C] (Tf = 1: shared by the frames, Tf = B: one per
// frame) at a uv G-buffer [B, H, W, 2], and its gradients.  u runs along the texture's width, v along its height, the
// top row first; texel (i, j) has its centre at u = (j + 0.5) / Tw, v = (i + 0.5) / Th (hill.h's convention).
//
// Rule, float32, every line one IEEE operation (the build has -ffp-contract=off); for u with T = Tw (v, Th alike):
//   clamp:  uc = min(max(u, 0), 1)            repeat:  uc = u - floor(u)   (may round to exactly 1)
//   x = uc * T;  x = x - 0.5;  fx = floor(x);  a = x - fx;  j0 = (int)fx;  j1 = j0 + 1
//   j0, j1 reduced into [0, T): clamped (clamp) or taken modulo T (repeat)
// fx lies in [-1, T - 1] for every finite u; the conversion clamps it to [-1, T] first and sends a NaN to -1, so no
// uv, finite or not, forms an address outside the texture.  Per channel
//   top = t[i0,j0] * (1 - a) + t[i0,j1] * a;  bot = t[i1,j0] * (1 - a) + t[i1,j1] * a;  out = top * (1 - b) + bot * b
// A pixel is sampled where mask != 0 (mask NULL: where both uv channels are finite); the others give exactly 0, carry
// no gradient and never form an address.
//
// Backward, one launch, with g = grad_texels[p, :] at sampled pixels:
//   grad_u = pass_u ? Tw * sum_c g_c * ((t[i0,j1] - t[i0,j0]) * (1 - b) + (t[i1,j1] - t[i1,j0]) * b) : 0
//   grad_v = pass_v ? Th * sum_c g_c * (bot_c - top_c) : 0         pass: 0 <= u <= 1 (clamp), always (repeat)
// is a gather in a fixed order: bit-identical from run to run.
//   grad_texture[i0,j0,c] += g_c * (1 - a) * (1 - b)   and likewise for the other three taps
// is a scatter-add with float atomics (the last bits may differ from run to run).  Its contention grows with the
// magnification: a 1024^2 frame over a 64^2 texture sends 256 pixels to each texel.  So a 256-thread workgroup owns a
// 16 x 16 screen tile, finds the bounding box of its sampled lanes' taps, and when the box holds at most
// kTexPatchTexels texels sums the tile's 4 * C * 256 terms in an LDS patch (ds_add_f32), then flushes the patch.  A box
// that does not fit (minification, scattered uv, a tile on the repeat seam of a large texture) adds straight to memory.

#ifndef DIRT_TEXTURE_PATCH
#define DIRT_TEXTURE_PATCH 576  // texels of the LDS patch (24 x 24); 0 builds the direct-atomics-only kernel (A/B)
#endif
constexpr int kTexPatchTexels = DIRT_TEXTURE_PATCH;
constexpr int kTexTile = 16;  // the backward's screen tile: kTexTile^2 == kLightThreads

// one coordinate of the rule: the two reduced tap indices and the weight of the second
struct TexAxis {
    int i0, i1;
    float a;
    bool pass;
};
constexpr TexAxis kTexNoAxis = {0, 0, 0.0f, false};  // of a lane that samples nothing
__device__ __forceinline__ TexAxis tex_axis(float u, int T, int wrap)
{
    TexAxis r;
    float uc;
    if (wrap == DIRT_TEXTURE_REPEAT) {
        uc = u - floorf(u);
        r.pass = true;
    } else {
        uc = fminf(fmaxf(u, 0.0f), 1.0f);
        r.pass = u >= 0.0f && u <= 1.0f;
    }
    float x = uc * (float)T;
    x = x - 0.5f;
    const float fx = floorf(x);
    r.a = x - fx;
    const int j0 = fx >= 0.0f ? (int)fminf(fx, (float)T) : -1;  // (a NaN compares false)
    const int j1 = j0 + 1;
    if (wrap == DIRT_TEXTURE_REPEAT) {
        r.i0 = ((j0 % T) + T) % T;
        r.i1 = ((j1 % T) + T) % T;
    } else {
        r.i0 = min(max(j0, 0), T - 1);
        r.i1 = min(max(j1, 0), T - 1);
    }
    return r;
}

__device__ __forceinline__ bool tex_sampled(const float *__restrict__ uv, const uint8_t *__restrict__ mask, int64_t p,
                                            float *u, float *v)
{
    *u = uv[p * 2];
    *v = uv[p * 2 + 1];
    return mask ? mask[p] != 0 : (isfinite(*u) && isfinite(*v));
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// ---- the per-level rules: a level is its first float t in the pixel's frame and its dimensions; the kernels below
// call them with one level, the texture itself, texture_mip_kernels.h with two

template <int C>
__device__ __forceinline__ void tex_bilinear(const float *__restrict__ t, int Tw, const TexAxis &ax, const TexAxis &ay,
                                             float *out)
{
    const float *t00 = t + ((int64_t)ay.i0 * Tw + ax.i0) * C, *t01 = t + ((int64_t)ay.i0 * Tw + ax.i1) * C;
    const float *t10 = t + ((int64_t)ay.i1 * Tw + ax.i0) * C, *t11 = t + ((int64_t)ay.i1 * Tw + ax.i1) * C;
    const float a = ax.a, b = ay.a, oma = 1.0f - a, omb = 1.0f - b;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float top = t00[c] * oma + t01[c] * a;
        const float bot = t10[c] * oma + t11[c] * a;
        out[c] = top * omb + bot * b;
    }
}

// the uv gradient of one level (Th x Tw) of a sampled pixel with upstream g
template <int C>
__device__ __forceinline__ void tex_grad_uv(const float *__restrict__ t, int Th, int Tw, const TexAxis &ax,
                                            const TexAxis &ay, const float *g, float *gu, float *gv)
{
    const float a = ax.a, b = ay.a, oma = 1.0f - a, omb = 1.0f - b;
    const int64_t o00 = ((int64_t)ay.i0 * Tw + ax.i0) * C, o01 = ((int64_t)ay.i0 * Tw + ax.i1) * C;
    const int64_t o10 = ((int64_t)ay.i1 * Tw + ax.i0) * C, o11 = ((int64_t)ay.i1 * Tw + ax.i1) * C;
    float su = 0.0f, sv = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float t00 = t[o00 + c], t01 = t[o01 + c], t10 = t[o10 + c], t11 = t[o11 + c];
        const float du = (t01 - t00) * omb + (t11 - t10) * b;
        const float top = t00 * oma + t01 * a;
        const float bot = t10 * oma + t11 * a;
        su += g[c] * du;  // (the first sum adds to +0: exact)
        sv += g[c] * (bot - top);
    }
    *gu = ax.pass ? (float)Tw * su : 0.0f;
    *gv = ay.pass ? (float)Th * sv : 0.0f;
}

// the four taps of one level of one lane, added with the level weight wl (1.0f: one level, the product is the tap
// itself) to dst: the level's first float in global memory (bw = the level's width, r0 = c0 = 0) or an LDS patch over
// the box of rows r0.., columns c0.., bw wide
template <int C>
__device__ __forceinline__ void tex_add_taps(float *dst, int r0, int c0, int bw, const TexAxis &ax, const TexAxis &ay,
                                             const float *g, float wl)
{
    const float a = ax.a, b = ay.a, oma = 1.0f - a, omb = 1.0f - b;
    const int64_t o00 = ((int64_t)(ay.i0 - r0) * bw + (ax.i0 - c0)) * C,
                  o01 = ((int64_t)(ay.i0 - r0) * bw + (ax.i1 - c0)) * C;
    const int64_t o10 = ((int64_t)(ay.i1 - r0) * bw + (ax.i0 - c0)) * C,
                  o11 = ((int64_t)(ay.i1 - r0) * bw + (ax.i1 - c0)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        atomicAdd(dst + o00 + c, g[c] * oma * omb * wl);
        atomicAdd(dst + o01 + c, g[c] * a * omb * wl);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        atomicAdd(dst + o10 + c, g[c] * oma * b * wl);
        atomicAdd(dst + o11 + c, g[c] * a * b * wl);
    }
}

constexpr int kTexBoxEmpty = 0x7fffffff;  // what the four words of a box hold before the reduction
// The bounding box of the taps of a tile's lanes with `has`, reduced into LDS: box[0..3] = min row, -(max row), min
// column, -(max column), kTexBoxEmpty before (the barriers around it are the caller's).  i0 <= i1 and j0 <= j1 in
// clamp mode; on the repeat seam they swap, so both orders enter the box.
__device__ __forceinline__ void tex_box_reduce(bool has, const TexAxis &ax, const TexAxis &ay, int *box)
{
    constexpr int big = kTexBoxEmpty;
    const int lo_r = wave_min(has ? min(ay.i0, ay.i1) : big), hi_r = wave_min(has ? -max(ay.i0, ay.i1) : big);
    const int lo_c = wave_min(has ? min(ax.i0, ax.i1) : big), hi_c = wave_min(has ? -max(ax.i0, ax.i1) : big);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&box[0], lo_r);
        atomicMin(&box[1], hi_r);
        atomicMin(&box[2], lo_c);
        atomicMin(&box[3], hi_c);
    }
}

// The flush of an LDS patch over the box of rows r0.., columns c0.., bw wide, to its level (t, Tw wide): the nonzero
// elements once each, consecutive lanes on consecutive floats of a texel row.  Element e of the patch, its value s:
template <int C>
__device__ __forceinline__ void tex_flush_add(float s, int e, int r0, int c0, int bw, float *t, int Tw)
{
    const int run = bw * C, row = e / run;
    atomicAdd(t + ((int64_t)(r0 + row) * Tw + c0) * C + (e - row * run), s);
}
template <int C>
__device__ __forceinline__ void tex_flush_patch(const float *patch, int ne, int r0, int c0, int bw, float *t, int Tw)
{
    for (int e = threadIdx.x; e < ne; e += kLightThreads) {
        const float s = patch[e];
        if (s != 0.0f) tex_flush_add<C>(s, e, r0, c0, bw, t, Tw);
    }
}

template <int C>
__global__ __launch_bounds__(kLightThreads) void texture_sample_fwd_kernel(
    const float *__restrict__ texture, int64_t frame_stride, int Th, int Tw, const float *__restrict__ uv,
    const uint8_t *__restrict__ mask, int64_t hw, int64_t n, int wrap, float *__restrict__ texels,
    uint8_t *__restrict__ valid)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float u, v;
    const bool ok = tex_sampled(uv, mask, p, &u, &v);
    float out[C];
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = 0.0f;
    if (ok) {
        const TexAxis ax = tex_axis(u, Tw, wrap), ay = tex_axis(v, Th, wrap);
        tex_bilinear<C>(texture + (p / hw) * frame_stride, Tw, ax, ay, out);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) texels[p * C + c] = out[c];
    valid[p] = ok ? 1 : 0;
}

// One workgroup per 16 x 16 screen tile of one frame (blockIdx.x = (frame * tiles_y + tile_y) * tiles_x + tile_x).
template <int C>
__global__ __launch_bounds__(kLightThreads) void texture_sample_bwd_kernel(
    const float *__restrict__ texture, int64_t frame_stride, int Th, int Tw, const float *__restrict__ uv,
    const uint8_t *__restrict__ mask, int H, int W, int tiles_x, int tiles_y, int wrap,
    const float *__restrict__ grad, float *__restrict__ grad_texture, float *__restrict__ grad_uv)
{
    __shared__ float s_patch[(kTexPatchTexels > 0 ? kTexPatchTexels : 1) * C];
    __shared__ int s_box[4];

    const int tx = (int)(blockIdx.x % (unsigned)tiles_x);
    const int64_t rest = blockIdx.x / (unsigned)tiles_x;
    const int ty = (int)(rest % tiles_y);
    const int64_t frame = rest / tiles_y;
    const int y = ty * kTexTile + (int)(threadIdx.x / kTexTile), x = tx * kTexTile + (int)(threadIdx.x % kTexTile);
    const bool inside = y < H && x < W;
    const int64_t p = (frame * H + (inside ? y : 0)) * W + (inside ? x : 0);

    float u = 0.0f, v = 0.0f;
    const bool ok = inside && tex_sampled(uv, mask, p, &u, &v);
    TexAxis ax = kTexNoAxis, ay = ax;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = 0.0f;
    if (ok) {
        ax = tex_axis(u, Tw, wrap);
        ay = tex_axis(v, Th, wrap);
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = grad[p * C + c];
    }
    // The uv gradient and the direct taps stay inline here: they share these four offsets, and tex_grad_uv plus
    // tex_add_taps, which form them once each, measured 0.4 to 0.6 % slower in this kernel.
    const float a = ax.a, b = ay.a, oma = 1.0f - a, omb = 1.0f - b;
    const int64_t fbase = frame * frame_stride;
    const int64_t o00 = fbase + ((int64_t)ay.i0 * Tw + ax.i0) * C, o01 = fbase + ((int64_t)ay.i0 * Tw + ax.i1) * C;
    const int64_t o10 = fbase + ((int64_t)ay.i1 * Tw + ax.i0) * C, o11 = fbase + ((int64_t)ay.i1 * Tw + ax.i1) * C;

    if (grad_uv && inside) {
        float gu = 0.0f, gv = 0.0f;
        if (ok) {
            float su = 0.0f, sv = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t00 = texture[o00 + c], t01 = texture[o01 + c], t10 = texture[o10 + c],
                            t11 = texture[o11 + c];
                const float du = (t01 - t00) * omb + (t11 - t10) * b;
                const float top = t00 * oma + t01 * a;
                const float bot = t10 * oma + t11 * a;
                su += g[c] * du;  // (the first sum adds to +0: exact)
                sv += g[c] * (bot - top);
            }
            if (ax.pass) gu = (float)Tw * su;
            if (ay.pass) gv = (float)Th * sv;
        }
        grad_uv[p * 2] = gu;
        grad_uv[p * 2 + 1] = gv;
    }
    if (!grad_texture) return;  // (uniform)

    float *gt = grad_texture + fbase;
    if (kTexPatchTexels > 0) {
        if (threadIdx.x < 4) s_box[threadIdx.x] = kTexBoxEmpty;
        __syncthreads();
        tex_box_reduce(ok, ax, ay, s_box);
        __syncthreads();
        const int r0 = s_box[0], c0 = s_box[2];
        if (r0 == kTexBoxEmpty) return;  // no sampled pixel in the tile (uniform)
        const int bh = -s_box[1] - r0 + 1, bw = -s_box[3] - c0 + 1;
        if ((int64_t)bh * bw <= kTexPatchTexels) {
            const int ne = bh * bw * C;
            for (int e = threadIdx.x; e < ne; e += kLightThreads) s_patch[e] = 0.0f;
            __syncthreads();
            if (ok) tex_add_taps<C>(s_patch, r0, c0, bw, ax, ay, g, 1.0f);
            __syncthreads();
            tex_flush_patch<C>(s_patch, ne, r0, c0, bw, gt, Tw);
            return;
        }
    }
    if (ok) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            atomicAdd(grad_texture + o00 + c, g[c] * oma * omb);
            atomicAdd(grad_texture + o01 + c, g[c] * a * omb);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            atomicAdd(grad_texture + o10 + c, g[c] * oma * b);
            atomicAdd(grad_texture + o11 + c, g[c] * a * b);
        }
    }
}
