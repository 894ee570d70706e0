// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after texture_kernels.h
// (tex_axis, tex_box_reduce, tex_flush_add, kTexPatchTexels, kTexTile) and shade_lights_kernels.h (sl_wave_sum, kSlWaves).  Not
// a standalone header.
//
// deferred.sample_shadow: the receiver side of a shadow map.  depth [Sf, Sh, Sw] (Sf = 1: shared by the frames, Sf = B:
// one per frame) holds the light's clip-space z BEFORE the divide, +inf where nothing was drawn; positions [B, H, W, 3]
// is the world-position G-buffer; M is the light's matrix [4][4] (shared) or [B][4][4], row vectors: clip = [p, 1] @ M.
// A pixel is sampled where mask != 0 (mask NULL: where its three position channels are finite); the others give
// visibility exactly 0, valid 0, carry no gradient and form no address.
//
// Rule, float32, every line one IEEE operation (the build has -ffp-contract=off and a correctly rounded divide); for a
// sampled pixel with position p, j = 0..3:
//   c_j = ((p0 * M[0][j] + p1 * M[1][j]) + p2 * M[2][j]) + M[3][j]                       (cx, cy, cz, cw)
//   front = cw > 0;  iw = 1 / cw
//   u = (cx * iw) * 0.5 + 0.5;  v = 0.5 - (cy * iw) * 0.5          (row 0 of the map is its top: rule R1, y up)
//   inside = front && 0 <= u <= 1 && 0 <= v <= 1                    (a NaN compares false)
// A sampled pixel that is not inside is lit: visibility 1, no gradient, no address.  For an inside pixel the taps and
// weights (i0, i1, b) = tex_axis(v, Sh, clamp), (j0, j1, a) = tex_axis(u, Sw, clamp); zc = cz - bias; per tap, d its
// depth texel:
//   softness == 0:  s = d >= zc ? 1 : 0
//   softness  > 0:  t = (d - zc) * (1 / softness) + 1;  s = t < 0 ? 0 : (t > 1 ? 1 : t)   (selects: a NaN stays one)
//   visibility = (s00 * (1 - a) + s01 * a) * (1 - b) + (s10 * (1 - a) + s11 * a) * b
// (1 / softness is one float32 division on the host.)
//
// Backward, g the upstream cotangent of an inside pixel, oma = 1 - a, omb = 1 - b, is = 1 / softness; a tap passes
// where softness > 0, its texel is finite and 0 <= t <= 1 (torch.clamp's inclusive rule), m its pass flag as 0 / 1:
//   grad_depth[tap] += ((g * wa) * wb) * is         at passing taps, (wa, wb) = (oma | a, omb | b): float atomics
//   mt = m00 * oma + m01 * a;  mb = m10 * oma + m11 * a;  g_cz = -((g * (mt * omb + mb * b)) * is)
//   g_u = pass_u ? Sw * (g * ((s01 - s00) * omb + (s11 - s10) * b)) : 0
//   g_v = pass_v ? Sh * (g * ((s10 * oma + s11 * a) - (s00 * oma + s01 * a))) : 0        (pass: tex_axis's)
//   nx = g_u * 0.5;  ny = g_v * -0.5;  g_cx = nx * iw;  g_cy = ny * iw
//   g_cw = (-(nx * cx + ny * cy) * iw) * iw                                               (d (1 / cw) included)
//   grad_p[r] = ((g_cx * M[r][0] + g_cy * M[r][1]) + g_cz * M[r][2]) + g_cw * M[r][3]
//   grad_M[r][j] = sum over pixels of p_r * g_c[j],  grad_M[3][j] = sum over pixels of g_c[j]
// grad_p is a gather in a fixed order: bit-identical from run to run, exactly 0 at unsampled and non-inside pixels.
// No product with an infinity is formed: a pixel that is not inside contributes the constant 0 everywhere.
//
// Kernels.  Forward: one thread per pixel.  Backward: one workgroup of 256 threads per 16 x 16 screen tile of one frame
// (texture_sample_bwd_kernel's grid).  With kParams each thread's sixteen matrix terms are summed over the wave by
// sl_wave_sum's butterfly, the four waves' sums added in wave order, and the tile's sixteen partial sums written to
// workspace[frame][tile][16] with plain stores; shadow_reduce_kernel, launched after it on the same stream (the
// kernel boundary is the hand-off), then sums column j: per frame, thread t adds tiles t, t + 256, ... in that order,
// the butterfly and the four waves in order follow; a per-frame matrix is written per frame, a shared one adds the
// frames in frame order.  No float atomics, no flag, no spin: grad_M is bit-identical from run to run.  Every row the
// second kernel reads was written by the first: the workspace needs no clearing.  Without kParams neither the sums,
// their LDS nor the second launch exist.  The depth gradient goes through texture_sample_bwd_kernel's LDS patch: the
// tile's inside lanes reduce the box of their taps (tex_box_reduce); a box of at most kTexPatchTexels texels is
// summed in LDS (ds_add_f32) and flushed once (tex_flush_patch<1>'s loop over tex_flush_add<1>), a larger one adds
// straight to memory.  All offsets 64-bit.

constexpr int kShadowSums = 16;  // the light matrix, row-major

struct ShadowArgs {
    const float *matrix;  // [4][4], or [B][4][4] with matrix_pf
    int matrix_pf;
    float bias, softness, inv_softness;  // inv_softness = 1 / softness (unused at softness == 0)
};

// the clip coordinates of one position and what the rule derives from them
struct ShadowClip {
    float cx, cy, cz, cw, iw, u, v;
    bool inside;
};
__device__ __forceinline__ ShadowClip shadow_clip(float3 p, const float *__restrict__ M)
{
    float c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = ((p.x * M[j] + p.y * M[4 + j]) + p.z * M[8 + j]) + M[12 + j];
    ShadowClip r;
    r.cx = c[0];
    r.cy = c[1];
    r.cz = c[2];
    r.cw = c[3];
    r.iw = 1.0f / r.cw;
    r.u = (r.cx * r.iw) * 0.5f + 0.5f;
    r.v = 0.5f - (r.cy * r.iw) * 0.5f;
    r.inside = r.cw > 0.0f && r.u >= 0.0f && r.u <= 1.0f && r.v >= 0.0f && r.v <= 1.0f;
    return r;
}

__device__ __forceinline__ bool shadow_sampled(const float *__restrict__ positions, const uint8_t *__restrict__ mask,
                                               int64_t p, float3 *pos)
{
    *pos = ld3(positions + p * 3);
    return mask ? mask[p] != 0 : finite3(*pos);
}

// one tap: its lit fraction s and whether the ramp's gradient passes
struct ShadowTap {
    float s;
    bool pass;
};
__device__ __forceinline__ ShadowTap shadow_tap(float d, float zc, const ShadowArgs &A)
{
    ShadowTap r;
    if (A.softness > 0.0f) {
        const float t = (d - zc) * A.inv_softness + 1.0f;
        r.s = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
        r.pass = isfinite(d) && t >= 0.0f && t <= 1.0f;
    } else {
        r.s = d >= zc ? 1.0f : 0.0f;
        r.pass = false;
    }
    return r;
}

__global__ __launch_bounds__(kLightThreads) void shadow_sample_fwd_kernel(
    const float *__restrict__ depth, int64_t frame_stride, int Sh, int Sw, const float *__restrict__ positions,
    const uint8_t *__restrict__ mask, int64_t hw, int64_t n, ShadowArgs A, float *__restrict__ visibility,
    uint8_t *__restrict__ valid)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float3 pos;
    const bool ok = shadow_sampled(positions, mask, p, &pos);
    float out = 0.0f;
    if (ok) {
        const int64_t frame = p / hw;
        const ShadowClip c = shadow_clip(pos, A.matrix + (A.matrix_pf ? frame * 16 : 0));
        out = 1.0f;
        if (c.inside) {
            const TexAxis ax = tex_axis(c.u, Sw, DIRT_TEXTURE_CLAMP), ay = tex_axis(c.v, Sh, DIRT_TEXTURE_CLAMP);
            const float *t = depth + frame * frame_stride;
            const float zc = c.cz - A.bias;
            const float s00 = shadow_tap(t[(int64_t)ay.i0 * Sw + ax.i0], zc, A).s,
                        s01 = shadow_tap(t[(int64_t)ay.i0 * Sw + ax.i1], zc, A).s,
                        s10 = shadow_tap(t[(int64_t)ay.i1 * Sw + ax.i0], zc, A).s,
                        s11 = shadow_tap(t[(int64_t)ay.i1 * Sw + ax.i1], zc, A).s;
            const float a = ax.a, b = ay.a, oma = 1.0f - a, omb = 1.0f - b;
            const float top = s00 * oma + s01 * a;
            const float bot = s10 * oma + s11 * a;
            out = top * omb + bot * b;
        }
    }
    visibility[p] = out;
    valid[p] = ok ? 1 : 0;
}

// the four passing taps of one lane added to dst: the map's frame in global memory (bw = Sw, r0 = c0 = 0) or an LDS
// patch over the box of rows r0.., columns c0.., bw wide.  tex_add_taps adds all four; here each tap has its own flag.
__device__ __forceinline__ void shadow_add_taps(float *dst, int r0, int c0, int bw, const TexAxis &ax, const TexAxis &ay,
                                                float g, float is, const bool *m)
{
    const float a = ax.a, b = ay.a, oma = 1.0f - a, omb = 1.0f - b;
    if (m[0]) atomicAdd(dst + ((int64_t)(ay.i0 - r0) * bw + (ax.i0 - c0)), g * oma * omb * is);
    if (m[1]) atomicAdd(dst + ((int64_t)(ay.i0 - r0) * bw + (ax.i1 - c0)), g * a * omb * is);
    if (m[2]) atomicAdd(dst + ((int64_t)(ay.i1 - r0) * bw + (ax.i0 - c0)), g * oma * b * is);
    if (m[3]) atomicAdd(dst + ((int64_t)(ay.i1 - r0) * bw + (ax.i1 - c0)), g * a * b * is);
}

// One workgroup per 16 x 16 screen tile of one frame (blockIdx.x = (frame * tiles_y + tile_y) * tiles_x + tile_x).
template <bool kParams>
__global__ __launch_bounds__(kLightThreads) void shadow_sample_bwd_kernel(
    const float *__restrict__ depth, int64_t frame_stride, int Sh, int Sw, const float *__restrict__ positions,
    const uint8_t *__restrict__ mask, int H, int W, int tiles_x, int tiles_y, ShadowArgs A,
    const float *__restrict__ grad, float *__restrict__ grad_depth, float *__restrict__ grad_positions,
    float *__restrict__ partial)
{
    __shared__ float s_patch[kTexPatchTexels > 0 ? kTexPatchTexels : 1];
    __shared__ int s_box[4];
    __shared__ float wave_sums[kParams ? kSlWaves : 1][kParams ? kShadowSums : 1];

    const int tx = (int)(blockIdx.x % (unsigned)tiles_x);
    const int64_t rest = blockIdx.x / (unsigned)tiles_x;
    const int ty = (int)(rest % tiles_y);
    const int64_t frame = rest / tiles_y;
    const int y = ty * kTexTile + (int)(threadIdx.x / kTexTile), x = tx * kTexTile + (int)(threadIdx.x % kTexTile);
    const bool in_frame = y < H && x < W;
    const int64_t p = (frame * H + (in_frame ? y : 0)) * W + (in_frame ? x : 0);
    const float *M = A.matrix + (A.matrix_pf ? frame * 16 : 0);
    const float *t = depth + frame * frame_stride;

    float3 pos = make_float3(0.0f, 0.0f, 0.0f);
    const bool ok = in_frame && shadow_sampled(positions, mask, p, &pos);
    ShadowClip c;
    c.inside = false;
    if (ok) c = shadow_clip(pos, M);
    const bool has = ok && c.inside;  // the lanes with taps, and the only ones with a gradient
    TexAxis ax = kTexNoAxis, ay = ax;
    float gc[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // the adjoint of (cx, cy, cz, cw)
    float g = 0.0f;
    bool m[4] = {false, false, false, false};
    if (has) {
        ax = tex_axis(c.u, Sw, DIRT_TEXTURE_CLAMP);
        ay = tex_axis(c.v, Sh, DIRT_TEXTURE_CLAMP);
        g = grad[p];
        const float zc = c.cz - A.bias;
        const ShadowTap t00 = shadow_tap(t[(int64_t)ay.i0 * Sw + ax.i0], zc, A),
                        t01 = shadow_tap(t[(int64_t)ay.i0 * Sw + ax.i1], zc, A),
                        t10 = shadow_tap(t[(int64_t)ay.i1 * Sw + ax.i0], zc, A),
                        t11 = shadow_tap(t[(int64_t)ay.i1 * Sw + ax.i1], zc, A);
        m[0] = t00.pass;
        m[1] = t01.pass;
        m[2] = t10.pass;
        m[3] = t11.pass;
        if (grad_positions || kParams) {
            const float a = ax.a, b = ay.a, oma = 1.0f - a, omb = 1.0f - b;
            const float mt = (m[0] ? 1.0f : 0.0f) * oma + (m[1] ? 1.0f : 0.0f) * a;
            const float mb = (m[2] ? 1.0f : 0.0f) * oma + (m[3] ? 1.0f : 0.0f) * a;
            gc[2] = A.softness > 0.0f ? -((g * (mt * omb + mb * b)) * A.inv_softness) : 0.0f;
            const float du = (t01.s - t00.s) * omb + (t11.s - t10.s) * b;
            const float top = t00.s * oma + t01.s * a;
            const float bot = t10.s * oma + t11.s * a;
            const float gu = ax.pass ? (float)Sw * (g * du) : 0.0f;
            const float gv = ay.pass ? (float)Sh * (g * (bot - top)) : 0.0f;
            const float nx = gu * 0.5f, ny = gv * -0.5f;
            gc[0] = nx * c.iw;
            gc[1] = ny * c.iw;
            gc[3] = (-(nx * c.cx + ny * c.cy) * c.iw) * c.iw;
        }
    }
    if (grad_positions && in_frame) {
        float3 gp = make_float3(0.0f, 0.0f, 0.0f);
        if (has) {
            gp.x = ((gc[0] * M[0] + gc[1] * M[1]) + gc[2] * M[2]) + gc[3] * M[3];
            gp.y = ((gc[0] * M[4] + gc[1] * M[5]) + gc[2] * M[6]) + gc[3] * M[7];
            gp.z = ((gc[0] * M[8] + gc[1] * M[9]) + gc[2] * M[10]) + gc[3] * M[11];
        }
        st3(grad_positions + p * 3, gp);
    }
    if (kParams) {
        // (a lane without taps contributes the constant 0: its position may be infinite)
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const float pr[4] = {pos.x, pos.y, pos.z, 1.0f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float term = has ? (r < 3 ? pr[r] * gc[j] : gc[j]) : 0.0f;
                const float s = sl_wave_sum(term);
                if (lane == 0) wave_sums[wave][r * 4 + j] = s;
            }
        }
        __syncthreads();
        if (threadIdx.x < kShadowSums) {
            float s = wave_sums[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kSlWaves; ++w) s += wave_sums[w][threadIdx.x];
            partial[(int64_t)blockIdx.x * kShadowSums + threadIdx.x] = s;
        }
    }
    if (!grad_depth || !(A.softness > 0.0f)) return;  // (uniform)

    const bool adds = has && (m[0] || m[1] || m[2] || m[3]);
    float *gt = grad_depth + frame * frame_stride;
    if (kTexPatchTexels > 0) {
        if (threadIdx.x < 4) s_box[threadIdx.x] = kTexBoxEmpty;
        __syncthreads();
        tex_box_reduce(adds, ax, ay, s_box);
        __syncthreads();
        const int r0 = s_box[0], c0 = s_box[2];
        if (r0 == kTexBoxEmpty) return;  // no passing tap in the tile (uniform)
        const int bh = -s_box[1] - r0 + 1, bw = -s_box[3] - c0 + 1;
        if ((int64_t)bh * bw <= kTexPatchTexels) {
            const int ne = bh * bw;
            for (int e = threadIdx.x; e < ne; e += kLightThreads) s_patch[e] = 0.0f;
            __syncthreads();
            if (adds) shadow_add_taps(s_patch, r0, c0, bw, ax, ay, g, A.inv_softness, m);
            __syncthreads();
            // (tex_flush_patch<1>'s loop, written out: a second caller of that function moves the schedule of
            // texture_sample_bwd_kernel<1>'s own flush loop, and existing listings stay as they are)
            for (int e = threadIdx.x; e < ne; e += kLightThreads) {
                const float s = s_patch[e];
                if (s != 0.0f) tex_flush_add<1>(s, e, r0, c0, bw, gt, Sw);
            }
            return;
        }
    }
    if (adds) shadow_add_taps(gt, 0, 0, Sw, ax, ay, g, A.inv_softness, m);
}

// One workgroup per element j of the matrix (blockIdx.x = j = r * 4 + column): the column sum of the partial rows.
__global__ __launch_bounds__(kSlThreads) void shadow_reduce_kernel(const float *__restrict__ partial, int B,
                                                                    int64_t tiles, int matrix_pf,
                                                                    float *__restrict__ grad_matrix)
{
    __shared__ float wave_sums[kSlWaves];
    const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float total = 0.0f;
    for (int64_t frame = 0; frame < B; ++frame) {
        float s = 0.0f;
        for (int64_t c = tid; c < tiles; c += kSlThreads) s += partial[(frame * tiles + c) * kShadowSums + j];
        s = sl_wave_sum(s);
        if (lane == 0) wave_sums[wave] = s;
        __syncthreads();
        float f = wave_sums[0];
#pragma unroll
        for (int w = 1; w < kSlWaves; ++w) f += wave_sums[w];
        __syncthreads();
        if (matrix_pf) {
            if (tid == 0) grad_matrix[frame * kShadowSums + j] = f;
        } else {
            total = frame == 0 ? f : total + f;
        }
    }
    if (!matrix_pf && tid == 0) grad_matrix[j] = total;
}
