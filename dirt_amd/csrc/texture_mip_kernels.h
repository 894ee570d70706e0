// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after texture_kernels.h, where
// every per-level rule lives (its tex_* functions).  Not a standalone header.  Here are the chain, the level of detail,
// the blend of two levels and a tile's two boxes.
//
// Mipmapped deferred texturing: a box-filtered mip chain of a texture [Tf, Th, Tw, C], packed as [Tf, N, C] with the
// levels in order, each row-major, and the trilinear lookup of that chain at a uv G-buffer [B, H, W, 2].
//
// Chain.  Level 0 is the texture; level k + 1 exists while level k has every dimension even or 1 and not both 1, with
// dimensions max(1, T / 2) -- so level k is max(1, Th >> k) x max(1, Tw >> k) and an odd dimension > 1 ends the chain.
//   both dimensions >= 2:  t'[i,j] = ((t[2i,2j] + t[2i,2j+1]) + (t[2i+1,2j] + t[2i+1,2j+1])) * 0.25
//   one dimension 1:       t'[j]   = (t[2j] + t[2j+1]) * 0.5 along the other
// One launch per level (after a copy of level 0): every level-k texel is that pairwise tree over its block, the build
// runs once per texture and step rather than per pixel, and the levels past the first few are too small to matter.
// Its backward is one gather per level-0 element in a fixed order, coarsest level first:
//   acc = g[L-1][i >> (L-1), j >> (L-1)];  for k = L-2 .. 0:  acc = acc * w_k + g[k][i >> k, j >> k]
// with w_k the forward's box weight from level k to k + 1 (0.25 or 0.5): no atomics, no scratch buffer, the incoming
// gradient is only read, and the result is bit-identical from run to run.
//
// Level of detail of a sampled pixel (y, x), float32, every line one IEEE operation, from the raw uv (before any wrap):
//   x-difference d = uv[y,x+1] - uv[y,x] if x + 1 < W and that neighbour is sampled, else uv[y,x] - uv[y,x-1] if
//   x >= 1 and that neighbour is sampled, else 0; the y-difference alike
//   du = d_u * Tw;  dv = d_v * Th;  q = du * du + dv * dv;  rho2 = fmax(qx, qy)   (a NaN loses against a number)
//   rho2 = m * 2^e with m in [1, 2), both from the float's bit fields;  lod = 0.5 * (e + (m - 1))
//   lod = 0 unless rho2 >= 1 (0, subnormals, NaN);  lod = L - 1 when rho2 is inf
// (piecewise linear in place of log2: exact at powers of two, monotone, continuous, within 0.044 of 0.5 * log2(rho2).)
// An explicit lod buffer replaces all of that (a NaN in it becomes 0).  Then lod = lod + lod_bias, clamped to
// [0, L - 1].  The lod never carries a gradient, neither to the uv nor to an explicit lod.
//
// Trilinear: k0 = (int)floor(lod), f = lod - k0, k1 = min(k0 + 1, L - 1); s_k = tex_bilinear at level k (T = T_k, the
// same wrap);  out = s_k0 * (1 - f) + s_k1 * f, and out = s_k0 without reading level k1 when
// f == 0.  The forward stores each pixel's final lod ([B, H, W], 0 at unsampled pixels); the backward reads it back.
//
// Backward, one launch, a 256-thread workgroup per 16 x 16 screen tile:
//   grad_uv = grad_uv(k0) * (1 - f) + grad_uv(k1) * f, each term tex_grad_uv with T_k (f == 0: grad_uv(k0) alone) -- a
//   gather in a fixed order, bit-identical from run to run;
//   grad_packed[level, tap, c] += g_c * w1 * w2 * wl, tex_add_taps with wl = 1 - f or f (four taps when f == 0), float
//   atomics: summed per tile in two LDS patches first (the tile's lowest level and the one above it) where
//   their boxes fit, straight to memory otherwise (see the kernel).
// Every packed offset is formed in 64 bits.

constexpr int kMaxMipLevels = DIRT_MAX_MIP_LEVELS;

// dimensions of a level and the offset, in texels, of its first texel inside a frame of the packed chain
struct MipLevel {
    int h, w;
    int64_t off;
};
__host__ __device__ __forceinline__ MipLevel mip_next(MipLevel l)
{
    MipLevel r;
    r.off = l.off + (int64_t)l.h * l.w;
    r.h = l.h > 1 ? l.h >> 1 : 1;
    r.w = l.w > 1 ? l.w >> 1 : 1;
    return r;
}
__host__ __device__ __forceinline__ MipLevel mip_level(int Th, int Tw, int k)
{
    MipLevel r = {Th, Tw, 0};
    for (int m = 0; m < k; ++m) r = mip_next(r);
    return r;
}

// ---- chain build

// level 0: texture [Tf, n0] -> packed [Tf, frame_stride] (floats)
__global__ __launch_bounds__(kLightThreads) void mip_copy_kernel(const float *__restrict__ texture, int64_t n0,
                                                                int64_t frame_stride, int64_t n,
                                                                float *__restrict__ packed)
{
    const int64_t e = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t f = e / n0;
    packed[f * frame_stride + (e - f * n0)] = texture[e];
}

// level k (sh x sw at src_off) -> level k + 1 (dh x dw at dst_off), offsets in floats inside a frame; one thread per
// destination float, n = Tf * dh * dw * C of them
__global__ __launch_bounds__(kLightThreads) void mip_down_kernel(float *packed, int64_t frame_stride, int64_t src_off,
                                                                int sh, int sw, int64_t dst_off, int dh, int dw, int C,
                                                                int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t per_frame = (int64_t)dh * dw * C;
    const int64_t f = e / per_frame, r = e - f * per_frame;
    const int64_t t = r / C;
    const int c = (int)(r - t * C);
    const int i = (int)(t / dw), j = (int)(t - (int64_t)i * dw);
    const float *src = packed + f * frame_stride + src_off + c;
    float out;
    if (sh >= 2 && sw >= 2) {
        const float *r0 = src + ((int64_t)(2 * i) * sw + 2 * j) * C, *r1 = r0 + (int64_t)sw * C;
        out = ((r0[0] + r0[C]) + (r1[0] + r1[C])) * 0.25f;
    } else {
        const float *r0 = src + (int64_t)(2 * (sh >= 2 ? i : j)) * C;  // (one dimension is 1: a row of texels)
        out = (r0[0] + r0[C]) * 0.5f;
    }
    packed[f * frame_stride + dst_off + r] = out;
}

// grad_packed [Tf, frame_stride] -> grad_texture [Tf, Th, Tw, C]; one thread per level-0 float
__global__ __launch_bounds__(kLightThreads) void mip_build_bwd_kernel(const float *__restrict__ grad_packed,
                                                                     int64_t frame_stride, int Th, int Tw, int C, int L,
                                                                     int64_t n, float *__restrict__ grad_texture)
{
    const int64_t e = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t per_frame = (int64_t)Th * Tw * C;
    const int64_t f = e / per_frame, r = e - f * per_frame;
    const int64_t t = r / C;
    const int c = (int)(r - t * C);
    const int i = (int)(t / Tw), j = (int)(t - (int64_t)i * Tw);
    const float *g = grad_packed + f * frame_stride + c;
    MipLevel lv = mip_level(Th, Tw, L - 1);
    float acc = g[(lv.off + (int64_t)(i >> (L - 1)) * lv.w + (j >> (L - 1))) * C];
    for (int k = L - 2; k >= 0; --k) {
        // level k from level k + 1: its dimensions double (a dimension of 1 below the first level it reached 1 stays)
        const int h = max(1, Th >> k), w = max(1, Tw >> k);
        lv.off -= (int64_t)h * w;
        lv.h = h;
        lv.w = w;
        const float wk = (h >= 2 && w >= 2) ? 0.25f : 0.5f;
        acc = acc * wk;
        acc = acc + g[(lv.off + (int64_t)(i >> k) * w + (j >> k)) * C];
    }
    grad_texture[e] = acc;
}

// ---- lookup

__device__ __forceinline__ float mip_q(float d_u, float d_v, int Th, int Tw)
{
    const float du = d_u * (float)Tw;
    const float dv = d_v * (float)Th;
    const float a = du * du, b = dv * dv;
    return a + b;
}

// the lod of the sampled pixel p = (y, x) of its frame, before the bias
__device__ __forceinline__ float mip_auto_lod(const float *__restrict__ uv, const uint8_t *__restrict__ mask,
                                              int64_t p, int x, int y, int H, int W, float u, float v, int Th, int Tw,
                                              int L)
{
    float dxu = 0.0f, dxv = 0.0f, dyu = 0.0f, dyv = 0.0f, un, vn;
    if (x + 1 < W && tex_sampled(uv, mask, p + 1, &un, &vn)) {
        dxu = un - u;
        dxv = vn - v;
    } else if (x >= 1 && tex_sampled(uv, mask, p - 1, &un, &vn)) {
        dxu = u - un;
        dxv = v - vn;
    }
    if (y + 1 < H && tex_sampled(uv, mask, p + W, &un, &vn)) {
        dyu = un - u;
        dyv = vn - v;
    } else if (y >= 1 && tex_sampled(uv, mask, p - W, &un, &vn)) {
        dyu = u - un;
        dyv = v - vn;
    }
    const float rho2 = fmaxf(mip_q(dxu, dxv, Th, Tw), mip_q(dyu, dyv, Th, Tw));
    if (!(rho2 >= 1.0f)) return 0.0f;
    if (isinf(rho2)) return (float)(L - 1);
    const uint32_t bits = __float_as_uint(rho2);
    const float e = (float)((int)(bits >> 23) - 127);
    const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);
    const float s = e + (m - 1.0f);
    return 0.5f * s;
}

__device__ __forceinline__ float mip_final_lod(float lod, float lod_bias, int L)
{
    lod = lod + lod_bias;
    return fminf(fmaxf(lod, 0.0f), (float)(L - 1));
}

// the two levels of a lod and the weight of the second
struct MipPick {
    MipLevel l0, l1;
    int k0;
    float f;
};
__device__ __forceinline__ MipPick mip_pick(float lod, int Th, int Tw, int L)
{
    MipPick r;
    const float fl = floorf(lod);
    const int k0 = min(max((int)fl, 0), L - 1);  // (lod is in [0, L - 1] already: the clamp costs nothing)
    r.f = lod - fl;
    r.k0 = k0;
    r.l0 = mip_level(Th, Tw, k0);
    r.l1 = k0 + 1 < L ? mip_next(r.l0) : r.l0;
    return r;
}

template <int C>
__global__ __launch_bounds__(kLightThreads) void texture_sample_mip_fwd_kernel(
    const float *__restrict__ packed, int64_t frame_stride, int Th, int Tw, int L, const float *__restrict__ uv,
    const uint8_t *__restrict__ mask, const float *__restrict__ lod_in, float lod_bias, int H, int W, int64_t n,
    int wrap, float *__restrict__ texels, uint8_t *__restrict__ valid, float *__restrict__ lod_out)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float u, v;
    const bool ok = tex_sampled(uv, mask, p, &u, &v);
    float out[C];
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = 0.0f;
    float lod = 0.0f;
    if (ok) {
        const int64_t row = p / W;
        const int x = (int)(p - row * W), y = (int)(row % H);
        if (lod_in) {
            lod = lod_in[p];
            if (lod != lod) lod = 0.0f;
        } else {
            lod = mip_auto_lod(uv, mask, p, x, y, H, W, u, v, Th, Tw, L);
        }
        lod = mip_final_lod(lod, lod_bias, L);
        const MipPick pk = mip_pick(lod, Th, Tw, L);
        const float *t = packed + (row / H) * frame_stride;
        tex_bilinear<C>(t + pk.l0.off * C, pk.l0.w, tex_axis(u, pk.l0.w, wrap), tex_axis(v, pk.l0.h, wrap), out);
        if (pk.f != 0.0f) {
            float s1[C];
            tex_bilinear<C>(t + pk.l1.off * C, pk.l1.w, tex_axis(u, pk.l1.w, wrap), tex_axis(v, pk.l1.h, wrap), s1);
            const float omf = 1.0f - pk.f;
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = out[c] * omf + s1[c] * pk.f;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) texels[p * C + c] = out[c];
    valid[p] = ok ? 1 : 0;
    lod_out[p] = lod;
}

#ifndef DIRT_TEXTURE_MIP_PATCH
// texels of LDS the two patches of a tile share; 0 builds direct atomics only (A/B).  A tile at up to 2 texels per
// pixel has a 33 x 33 box at level A and a 17 x 17 one at B, 1378 texels; 1408 is that rounded up to a multiple of 64
// (DESIGN.md 7i has the A/B against 768).
#define DIRT_TEXTURE_MIP_PATCH 1408
#endif
constexpr int kMipPatchTexels = DIRT_TEXTURE_MIP_PATCH;

// One workgroup per 16 x 16 screen tile of one frame (blockIdx.x = (frame * tiles_y + tile_y) * tiles_x + tile_x): a
// tile's lanes share their levels and a compact texel footprint.  grad_uv first, a gather per lane.  Then the tile
// takes its lowest k0 (level A) and the level above it (B), reduces the boxes of its lanes' taps at A (lanes with
// k0 = A) and at B (their second level, and the first level of lanes with k0 = B), tex_box_reduce each; the boxes
// share kMipPatchTexels texels of LDS, A served first, B from what A leaves.  A box that fits sums its taps in LDS and
// is flushed as the plain kernel's.  Taps at any other level, and those of a box that does not fit, go to memory.
template <int C>
__global__ __launch_bounds__(kLightThreads) void texture_sample_mip_bwd_kernel(
    const float *__restrict__ packed, int64_t frame_stride, int Th, int Tw, int L, const float *__restrict__ uv,
    const uint8_t *__restrict__ mask, const float *__restrict__ lod_saved, int H, int W, int tiles_x, int tiles_y,
    int wrap, const float *__restrict__ grad, float *__restrict__ grad_packed, float *__restrict__ grad_uv)
{
    __shared__ float s_patch[(kMipPatchTexels > 0 ? kMipPatchTexels : 1) * C];
    __shared__ int s_box[9];  // the lowest k0; then per level A, B: min row, -(max row), min column, -(max column)

    const int tx = (int)(blockIdx.x % (unsigned)tiles_x);
    const int64_t rest = blockIdx.x / (unsigned)tiles_x;
    const int ty = (int)(rest % tiles_y);
    const int64_t frame = rest / tiles_y;
    const int y = ty * kTexTile + (int)(threadIdx.x / kTexTile), x = tx * kTexTile + (int)(threadIdx.x % kTexTile);
    const bool inside = y < H && x < W;
    const int64_t p = (frame * H + (inside ? y : 0)) * W + (inside ? x : 0);
    float u = 0.0f, v = 0.0f;
    const bool ok = inside && tex_sampled(uv, mask, p, &u, &v);
    const int64_t fbase = frame * frame_stride;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = 0.0f;
    MipPick pk = mip_pick(0.0f, Th, Tw, L);
    if (ok) {
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = grad[p * C + c];
        pk = mip_pick(lod_saved[p], Th, Tw, L);
    }
    const bool two = ok && pk.f != 0.0f;
    const float omf = 1.0f - pk.f;

    if (grad_uv && inside) {
        float gu = 0.0f, gv = 0.0f;
        if (ok) {
            const float *t = packed + fbase;
            tex_grad_uv<C>(t + pk.l0.off * C, pk.l0.h, pk.l0.w, tex_axis(u, pk.l0.w, wrap),
                           tex_axis(v, pk.l0.h, wrap), g, &gu, &gv);
            if (two) {
                float gu1, gv1;
                tex_grad_uv<C>(t + pk.l1.off * C, pk.l1.h, pk.l1.w, tex_axis(u, pk.l1.w, wrap),
                               tex_axis(v, pk.l1.h, wrap), g, &gu1, &gv1);
                gu = gu * omf + gu1 * pk.f;
                gv = gv * omf + gv1 * pk.f;
            }
        }
        grad_uv[p * 2] = gu;
        grad_uv[p * 2 + 1] = gv;
    }
    if (!grad_packed) return;  // (uniform)

    float *gp = grad_packed + fbase;
    TexAxis ax0 = kTexNoAxis, ay0 = ax0, ax1 = ax0, ay1 = ax0;
    if (ok) {
        ax0 = tex_axis(u, pk.l0.w, wrap);
        ay0 = tex_axis(v, pk.l0.h, wrap);
    }
    if (two) {
        ax1 = tex_axis(u, pk.l1.w, wrap);
        ay1 = tex_axis(v, pk.l1.h, wrap);
    }
    const float w0 = two ? omf : 1.0f;

    if (kMipPatchTexels > 0) {
        if (threadIdx.x < 9) s_box[threadIdx.x] = kTexBoxEmpty;
        __syncthreads();
        const int kmin_w = wave_min(ok ? pk.k0 : kTexBoxEmpty);
        if ((threadIdx.x & 63) == 0) atomicMin(&s_box[0], kmin_w);
        __syncthreads();
        const int kA = s_box[0];
        if (kA == kTexBoxEmpty) return;  // no sampled pixel in the tile (uniform)
        // this lane's taps at level A and at level B
        const bool hasA = ok && pk.k0 == kA, firstB = ok && pk.k0 == kA + 1, hasB = firstB || (hasA && two);
        tex_box_reduce(hasA, ax0, ay0, s_box + 1);
        tex_box_reduce(hasB, firstB ? ax0 : ax1, firstB ? ay0 : ay1, s_box + 5);
        __syncthreads();
        const int rA = s_box[1], cA = s_box[3], hA = -s_box[2] - rA + 1, wA = -s_box[4] - cA + 1;
        const bool anyB = s_box[5] != kTexBoxEmpty;
        const int rB = anyB ? s_box[5] : 0, cB = anyB ? s_box[7] : 0;
        const int hB = anyB ? -s_box[6] - rB + 1 : 0, wB = anyB ? -s_box[8] - cB + 1 : 0;
        // A takes the budget first, B what A leaves: a tile whose finer box is too large still sums the coarser one
        const int64_t nA = (int64_t)hA * wA, nB = (int64_t)hB * wB;
        const bool inA = nA <= kMipPatchTexels, inB = anyB && nB <= kMipPatchTexels - (inA ? nA : 0);  // (uniform)
        if (inA || inB) {
            const int eA = inA ? (int)nA * C : 0, eB = inB ? (int)nB * C : 0;
            for (int e = threadIdx.x; e < eA + eB; e += kLightThreads) s_patch[e] = 0.0f;
            __syncthreads();
            if (hasA && inA) tex_add_taps<C>(s_patch, rA, cA, wA, ax0, ay0, g, w0);
            else if (firstB && inB) tex_add_taps<C>(s_patch + eA, rB, cB, wB, ax0, ay0, g, w0);
            else if (ok) tex_add_taps<C>(gp + pk.l0.off * C, 0, 0, pk.l0.w, ax0, ay0, g, w0);
            if (two) {
                if (hasA && inB) tex_add_taps<C>(s_patch + eA, rB, cB, wB, ax1, ay1, g, pk.f);
                else tex_add_taps<C>(gp + pk.l1.off * C, 0, 0, pk.l1.w, ax1, ay1, g, pk.f);
            }
            __syncthreads();
            // flush, both patches in one pass over their eA + eB floats (a tex_flush_patch per box costs 6 SGPRs)
            const MipLevel lA = mip_level(Th, Tw, kA), lB = mip_next(lA);
            for (int e = threadIdx.x; e < eA + eB; e += kLightThreads) {
                const float s = s_patch[e];
                if (s != 0.0f) {
                    const bool second = e >= eA;
                    const MipLevel &lv = second ? lB : lA;
                    tex_flush_add<C>(s, second ? e - eA : e, second ? rB : rA, second ? cB : cA, second ? wB : wA,
                                     gp + lv.off * C, lv.w);
                }
            }
            return;
        }
    }
    if (ok) tex_add_taps<C>(gp + pk.l0.off * C, 0, 0, pk.l0.w, ax0, ay0, g, w0);
    if (two) tex_add_taps<C>(gp + pk.l1.off * C, 0, 0, pk.l1.w, ax1, ay1, g, pk.f);
}
