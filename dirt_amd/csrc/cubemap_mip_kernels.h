// Part of dirt_raster.hip's translation unit: included inside its anonymous namespace after cubemap_kernels.h (the
// face rule: cube_sampled, cube_coord, cube_grad_direction) and texture_mip_kernels.h (the chain's layout and the
// level pick: mip_level, mip_next, mip_final_lod, mip_pick), with the per-level rules of texture_kernels.h under both
// (tex_bilinear, tex_add_taps, tex_box_reduce, tex_flush_add).  Not a standalone header.
//
// Seamless mip-mapped cube-map lookup: the trilinear lookup of a cube map's mip chain [Cf, 6, N, C] (each face's
// chain as texture_mip_kernels.h packs it, N = sum_k S_k^2, S_k = S >> k while S_k is even; Cf = 1: shared by the
// frames, Cf = B: one per frame) at a direction G-buffer [B, H, W, 3], and its gradients to the chain, the directions
// and an explicit level of detail.  The chain itself is built by mip_copy_kernel / mip_down_kernel with 6 * Cf frames.
//
// Rule, float32, every line one IEEE operation (the build has -ffp-contract=off); (x, y, z) a sampled direction:
//   face, ma, m, su, sv, u, v: cube_coord.
//   lod, explicit: the pixel's lod_in, a NaN counting as 0.
//   lod, automatic: P = (x / m, y / m, z / m), the point on the unit cube (continuous across the seams);
//     the x-difference e = P[y,x+1] - P[y,x] if x + 1 < W and that neighbour is sampled, else P[y,x] - P[y,x-1] if
//     x >= 1 and that neighbour is sampled, else 0; the y-difference alike;
//     h = 0.5 * S;  e = e * h per component;  q = ex * ex;  t = ey * ey;  q = q + t;  t = ez * ez;  q = q + t
//     rho2 = fmax(qx, qy);  then mip_auto_lod's tail: rho2 = m * 2^e from the bit fields, lod = 0.5 * (e + (m - 1)),
//     0 unless rho2 >= 1, L - 1 at inf.
//   lod = lod + lod_bias, clamped to [0, L - 1];  k0 = floor(lod), f = lod - k0, k1 = min(k0 + 1, L - 1).
//   taps at level k, T = S_k:  x = u * T;  x = x - 0.5;  fx = floor(x);  a = x - fx;  j0 = (int)fx;  j1 = j0 + 1, so
//     j0 in [-1, T - 1], j1 in [0, T]; i0, i1, b from v alike.  Not seamless: the four indices clamped to [0, T - 1]
//     (sample_cubemap's rule).  Seamless: a tap (i, j) is resolved in integers.  sc = 2 j + 1 - T, tc = 2 i + 1 - T,
//     and the inverse face table with major T gives its point:
//       +x: (T, -tc, -sc)  -x: (-T, -tc, sc)  +y: (sc, T, tc)  -y: (sc, -T, -tc)  +z: (sc, -tc, T)  -z: (-sc, -tc, -T)
//     both indices in range: texel (i, j) of the pixel's face;
//     one out of range (a coordinate of magnitude T + 1): that coordinate becomes +-T and the major axis, the old major
//       coordinate +-(T - 1), the third stays; the face table gives (face', sc', tc'), j' = (sc' + T - 1) / 2,
//       i' = (tc' + T - 1) / 2, exact integers in [0, T);
//     both out of range (a cube corner, at most one of the four taps): no texel; its value is
//       ((t_p + t_q) + t_r) * third, third = float32(1 / 3), p, q, r the other three taps in the order 00, 01, 10, 11.
//   s_k = tex_bilinear's three lines on the four tap values;  out = s_k0 * (1 - f) + s_k1 * f, and out = s_k0 without
//   reading level k1 when f == 0.
// Unsampled pixels (cube_sampled) give exactly 0, form no address, carry no gradient.  The forward stores the final
// lod ([B, H, W], 0 at unsampled pixels); the backward reads it back.
//
// Backward, one launch, a 256-thread workgroup per 16 x 16 screen tile, g = grad_texels[p, :]:
//   grad_packed: tex_add_taps' terms g_c * w1 * w2 * wl at the resolved texels, wl = 1 - f and f (1 with f == 0, the
//     four taps of k0 alone); a corner tap's term times third, to each of its three source texels.  Float atomics.
//   grad_directions: per level (gu, gv) in tex_grad_uv's difference form on the resolved tap values (the corner tap's
//     value is its mean; pass always true), blended gu = gu(k0) * (1 - f) + gu(k1) * f (f == 0: k0 alone), then
//     cube_grad_direction.  A gather in a fixed order, bit-identical from run to run.
//   grad_lod = pass ? sum_c g_c * (s_k1,c - s_k0,c) : 0, pass: lod_in not NaN and 0 <= lod_in + lod_bias <= L - 1.  At
//     an integer lod that is the derivative to the right (level k1 is read although the forward did not); k1 == k0
//     gives 0.  A gather too.
// The scatter per tile: the tile's lowest k0 is level A, the one above it B (as texture_sample_mip_bwd_kernel).  A
// level whose whole cube, 6 * S_k^2 texels, fits the LDS budget is summed in LDS as a whole: seams and corners cost
// nothing there.  Otherwise, when the tile's lanes at that level lie on one face with every tap in range and the box
// of their taps fits, the box is summed in LDS.  Otherwise the lanes add straight to memory.  A is served first, B
// from what A leaves, and both are flushed in one pass.  Every packed offset is formed in 64 bits.

#ifndef DIRT_CUBEMAP_MIP_PATCH
// texels of LDS that a tile's two levels share; 0 builds direct atomics only (A/B: DESIGN.md 7n)
#define DIRT_CUBEMAP_MIP_PATCH DIRT_TEXTURE_MIP_PATCH
#endif
constexpr int kCubeMipPatchTexels = DIRT_CUBEMAP_MIP_PATCH;

// the four taps of a pixel at one level, in the order 00, 01, 10, 11
struct CubeTaps {
    int face[4], idx[4];  // the resolved texel: its face and i * T + j on it; face -1: the corner tap (no texel)
    int r0, r1, c0, c1;   // the rows and columns on the pixel's own face: unreduced (seamless) or clamped
    float a, b;
};

// one coordinate of the tap rule, unreduced: j0 in [-1, T - 1] for u in [0, 1] (tex_axis' guard: a NaN goes to -1)
__device__ __forceinline__ int cube_mip_axis(float u, int T, float *a)
{
    float x = u * (float)T;
    x = x - 0.5f;
    const float fx = floorf(x);
    *a = x - fx;
    return fx >= 0.0f ? (int)fminf(fx, (float)(T - 1)) : -1;
}

// the texel that tap (i, j) of `face` at a level of T x T faces resolves to (the module comment's integer rule)
__device__ __forceinline__ void cube_mip_resolve(int face, int i, int j, int T, int *rface, int *ridx)
{
    const bool oi = i < 0 || i >= T, oj = j < 0 || j >= T;
    if (!oi && !oj) {
        *rface = face;
        *ridx = i * T + j;
        return;
    }
    if (oi && oj) {
        *rface = -1;
        *ridx = 0;
        return;
    }
    const int sc = 2 * j + 1 - T, tc = 2 * i + 1 - T;
    int x, y, z;
    switch (face) {
    case 0: x = T, y = -tc, z = -sc; break;
    case 1: x = -T, y = -tc, z = sc; break;
    case 2: x = sc, y = T, z = tc; break;
    case 3: x = sc, y = -T, z = -tc; break;
    case 4: x = sc, y = -tc, z = T; break;
    default: x = -sc, y = -tc, z = -T; break;
    }
    // the fold: the old major coordinate shrinks to +-(T - 1), the one past the edge (T + 1) is the new major
    const int old = face >> 1;
    if (old == 0) x = x < 0 ? 1 - T : T - 1;
    else if (old == 1) y = y < 0 ? 1 - T : T - 1;
    else z = z < 0 ? 1 - T : T - 1;
    int sc2, tc2;
    if (x > T || x < -T) {
        *rface = x < 0 ? 1 : 0;
        sc2 = x < 0 ? z : -z;
        tc2 = -y;
    } else if (y > T || y < -T) {
        *rface = y < 0 ? 3 : 2;
        sc2 = x;
        tc2 = y < 0 ? -z : z;
    } else {
        *rface = z < 0 ? 5 : 4;
        sc2 = z < 0 ? -x : x;
        tc2 = -y;
    }
    *ridx = ((tc2 + T - 1) >> 1) * T + ((sc2 + T - 1) >> 1);
}

__device__ __forceinline__ CubeTaps cube_mip_taps(const CubeCoord &cc, int T, bool seamless)
{
    CubeTaps t;
    t.c0 = cube_mip_axis(cc.u, T, &t.a);
    t.r0 = cube_mip_axis(cc.v, T, &t.b);
    t.c1 = t.c0 + 1;
    t.r1 = t.r0 + 1;
    if (!seamless) {
        t.c0 = max(t.c0, 0);
        t.r0 = max(t.r0, 0);
        t.c1 = min(t.c1, T - 1);
        t.r1 = min(t.r1, T - 1);
    }
    cube_mip_resolve(cc.face, t.r0, t.c0, T, &t.face[0], &t.idx[0]);
    cube_mip_resolve(cc.face, t.r0, t.c1, T, &t.face[1], &t.idx[1]);
    cube_mip_resolve(cc.face, t.r1, t.c0, T, &t.face[2], &t.idx[2]);
    cube_mip_resolve(cc.face, t.r1, t.c1, T, &t.face[3], &t.idx[3]);
    return t;
}

__device__ __forceinline__ float cube_mip_third() { return 1.0f / 3.0f; }  // float32(1 / 3), folded at compile time

// the four tap values of one level as a 2 x 2 x C texture q, the corner tap's the mean of the other three; chain is
// the pixel's frame of the packed chain, n_face the texels of one face's chain, off the level's first texel in it
template <int C>
__device__ __forceinline__ void cube_mip_gather(const float *__restrict__ chain, int64_t n_face, int64_t off,
                                                const CubeTaps &t, float *q)
{
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (t.face[n] >= 0) {
            const float *src = chain + ((int64_t)t.face[n] * n_face + off + t.idx[n]) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) q[n * C + c] = src[c];
        }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (t.face[n] < 0) {
            const int np = n == 0 ? 1 : 0, nq = n <= 1 ? 2 : 1, nr = n <= 2 ? 3 : 2;  // the other three, in order
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float s = q[np * C + c] + q[nq * C + c];
                s = s + q[nr * C + c];
                q[n * C + c] = s * cube_mip_third();
            }
        }
    }
}

constexpr TexAxis kCubeMipFirst = {0, 1, 0.0f, true};  // the axes of the 2 x 2 texture q, their weights filled in

template <int C>
__device__ __forceinline__ void cube_mip_bilinear(const float *q, const CubeTaps &t, float *out)
{
    TexAxis ax = kCubeMipFirst, ay = kCubeMipFirst;
    ax.a = t.a;
    ay.a = t.b;
    tex_bilinear<C>(q, 2, ax, ay, out);
}

// tex_grad_uv's lines on the tap values q of a level of T x T faces (tex_grad_uv itself scales by the width it also
// indexes with)
template <int C>
__device__ __forceinline__ void cube_mip_grad_uv(const float *q, int T, const CubeTaps &t, const float *g, float *gu,
                                                 float *gv)
{
    const float a = t.a, b = t.b, oma = 1.0f - a, omb = 1.0f - b;
    float su = 0.0f, sv = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float t00 = q[c], t01 = q[C + c], t10 = q[2 * C + c], t11 = q[3 * C + c];
        const float du = (t01 - t00) * omb + (t11 - t10) * b;
        const float top = t00 * oma + t01 * a;
        const float bot = t10 * oma + t11 * a;
        su += g[c] * du;  // (the first sum adds to +0: exact)
        sv += g[c] * (bot - top);
    }
    *gu = (float)T * su;
    *gv = (float)T * sv;
}

// the point of a sampled direction on the unit cube
__device__ __forceinline__ void cube_mip_point(float x, float y, float z, float *px, float *py, float *pz)
{
    const float m = fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z));  // (|ma| of cube_coord)
    *px = x / m;
    *py = y / m;
    *pz = z / m;
}

__device__ __forceinline__ float cube_mip_q(float ex, float ey, float ez, float h)
{
    ex = ex * h;
    ey = ey * h;
    ez = ez * h;
    float q = ex * ex;
    float t = ey * ey;
    q = q + t;
    t = ez * ez;
    q = q + t;
    return q;
}

// the difference of the rule along one screen axis: to the next pixel (at p + step) where `next` allows it and it is
// sampled, else from the previous one, else 0
__device__ __forceinline__ void cube_mip_difference(const float *__restrict__ directions,
                                                    const uint8_t *__restrict__ mask, int64_t p, int64_t step,
                                                    bool next, bool prev, float px, float py, float pz, float *ex,
                                                    float *ey, float *ez)
{
    float nx, ny, nz, qx, qy, qz;
    *ex = *ey = *ez = 0.0f;
    if (next && cube_sampled(directions, mask, p + step, &nx, &ny, &nz)) {
        cube_mip_point(nx, ny, nz, &qx, &qy, &qz);
        *ex = qx - px;
        *ey = qy - py;
        *ez = qz - pz;
    } else if (prev && cube_sampled(directions, mask, p - step, &nx, &ny, &nz)) {
        cube_mip_point(nx, ny, nz, &qx, &qy, &qz);
        *ex = px - qx;
        *ey = py - qy;
        *ez = pz - qz;
    }
}

// the lod of the sampled pixel p = (y, x) of its frame with direction (dx, dy, dz), before the bias
__device__ __forceinline__ float cube_mip_auto_lod(const float *__restrict__ directions,
                                                   const uint8_t *__restrict__ mask, int64_t p, int x, int y, int H,
                                                   int W, float dx, float dy, float dz, int S, int L)
{
    float px, py, pz, ex, ey, ez;
    cube_mip_point(dx, dy, dz, &px, &py, &pz);
    const float h = 0.5f * (float)S;
    cube_mip_difference(directions, mask, p, 1, x + 1 < W, x >= 1, px, py, pz, &ex, &ey, &ez);
    const float qx = cube_mip_q(ex, ey, ez, h);
    cube_mip_difference(directions, mask, p, W, y + 1 < H, y >= 1, px, py, pz, &ex, &ey, &ez);
    const float qy = cube_mip_q(ex, ey, ez, h);
    const float rho2 = fmaxf(qx, qy);
    // (mip_auto_lod's tail, which that function does not give apart from its uv differences)
    if (!(rho2 >= 1.0f)) return 0.0f;
    if (isinf(rho2)) return (float)(L - 1);
    const uint32_t bits = __float_as_uint(rho2);
    const float e = (float)((int)(bits >> 23) - 127);
    const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);
    const float s = e + (m - 1.0f);
    return 0.5f * s;
}

template <int C>
__global__ __launch_bounds__(kLightThreads) void cubemap_sample_mip_fwd_kernel(
    const float *__restrict__ packed, int64_t frame_stride, int64_t n_face, int S, int L,
    const float *__restrict__ directions, const uint8_t *__restrict__ mask, const float *__restrict__ lod_in,
    float lod_bias, int H, int W, int64_t n, int seamless, float *__restrict__ texels, uint8_t *__restrict__ valid,
    float *__restrict__ lod_out)
{
    const int64_t p = (int64_t)blockIdx.x * kLightThreads + threadIdx.x;
    if (p >= n) return;
    float dx, dy, dz;
    const bool ok = cube_sampled(directions, mask, p, &dx, &dy, &dz);
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
            lod = cube_mip_auto_lod(directions, mask, p, x, y, H, W, dx, dy, dz, S, L);
        }
        lod = mip_final_lod(lod, lod_bias, L);
        const MipPick pk = mip_pick(lod, S, S, L);
        const CubeCoord cc = cube_coord(dx, dy, dz);
        const float *chain = packed + (row / H) * frame_stride;
        float q[4 * C];
        CubeTaps t = cube_mip_taps(cc, pk.l0.w, seamless != 0);
        cube_mip_gather<C>(chain, n_face, pk.l0.off, t, q);
        cube_mip_bilinear<C>(q, t, out);
        if (pk.f != 0.0f) {
            float s1[C];
            t = cube_mip_taps(cc, pk.l1.w, seamless != 0);
            cube_mip_gather<C>(chain, n_face, pk.l1.off, t, q);
            cube_mip_bilinear<C>(q, t, s1);
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

// ---- the scatter: where a lane's four taps of one level go, as float offsets from a destination

// from the frame's first float of grad_packed
__device__ __forceinline__ void cube_mip_offsets_memory(const CubeTaps &t, int64_t n_face, int64_t off, int C,
                                                        int64_t *o)
{
#pragma unroll
    for (int n = 0; n < 4; ++n) o[n] = t.face[n] < 0 ? -1 : ((int64_t)t.face[n] * n_face + off + t.idx[n]) * C;
}
// from the first float of a whole level (6 faces of T x T) in LDS
__device__ __forceinline__ void cube_mip_offsets_whole(const CubeTaps &t, int T, int C, int64_t *o)
{
#pragma unroll
    for (int n = 0; n < 4; ++n) o[n] = t.face[n] < 0 ? -1 : (int64_t)((t.face[n] * T * T + t.idx[n]) * C);
}

// tex_add_taps' terms at the offsets o (-1: the corner tap, whose term goes, times third, to the other three)
template <int C>
__device__ __forceinline__ void cube_mip_add_taps(float *dst, const int64_t *o, float a, float b, const float *g,
                                                  float wl)
{
    const float oma = 1.0f - a, omb = 1.0f - b;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const float w1 = (n & 1) ? a : oma, w2 = (n & 2) ? b : omb;
        if (o[n] >= 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) atomicAdd(dst + o[n] + c, g[c] * w1 * w2 * wl);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float term = g[c] * w1 * w2 * wl * cube_mip_third();
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k != n) atomicAdd(dst + o[k] + c, term);
            }
        }
    }
}

// how a tile sums one of its two levels
enum CubeMipMode { kCubeMipMemory = 0, kCubeMipBox = 1, kCubeMipWhole = 2 };

// a lane's taps of one level, added where the tile sums that level: patch is the level's part of the LDS patch, box
// (min row, min column, width) its box there, gp the frame's first float of grad_packed
template <int C>
__device__ __forceinline__ void cube_mip_scatter(int mode, float *patch, int r0, int c0, int bw, float *gp,
                                                 int64_t n_face, MipLevel lv, const CubeTaps &t, const float *g,
                                                 float wl)
{
    int64_t o[4];
    if (mode == kCubeMipWhole) {
        cube_mip_offsets_whole(t, lv.w, C, o);
        cube_mip_add_taps<C>(patch, o, t.a, t.b, g, wl);
    } else if (mode == kCubeMipBox) {  // (every tap in range on the lane's own face: tex_add_taps itself)
        TexAxis ax = {t.c0, t.c1, t.a, true}, ay = {t.r0, t.r1, t.b, true};
        tex_add_taps<C>(patch, r0, c0, bw, ax, ay, g, wl);
    } else {
        cube_mip_offsets_memory(t, n_face, lv.off, C, o);
        cube_mip_add_taps<C>(gp, o, t.a, t.b, g, wl);
    }
}

constexpr int kCubeMipFaceShift = 14;  // a face above the columns of a box word: columns + 1 lie in [0, 8193]

// the box of a tile's lanes with `has` at one level through tex_box_reduce, the lanes' face riding above the columns:
// box[2] >> shift is the lowest face, -box[3] >> shift the highest
__device__ __forceinline__ void cube_mip_box_reduce(bool has, int face, const CubeTaps &t, int *box)
{
    const int fb = face << kCubeMipFaceShift;
    const TexAxis ax = {fb + t.c0 + 1, fb + t.c1 + 1, 0.0f, true}, ay = {t.r0, t.r1, 0.0f, true};
    tex_box_reduce(has, ax, ay, box);
}

// a tile's decision for one level from its reduced box: the mode, and the box (min row, min column, height, width)
struct CubeMipPlan {
    int mode, r0, c0, bh, bw, face;
    int64_t texels;  // of LDS it takes
};
__device__ __forceinline__ CubeMipPlan cube_mip_plan(const int *box, int T, int64_t budget)
{
    CubeMipPlan r = {kCubeMipMemory, 0, 0, 0, 0, 0, 0};
    if (box[0] == kTexBoxEmpty) return r;  // no lane at this level
    if ((int64_t)6 * T * T <= budget) {
        r.mode = kCubeMipWhole;
        r.texels = (int64_t)6 * T * T;
        return r;
    }
    const int lo = box[2], hi = -box[3];
    const int face = lo >> kCubeMipFaceShift;
    r.r0 = box[0];
    r.bh = -box[1] - r.r0 + 1;
    r.c0 = (lo & ((1 << kCubeMipFaceShift) - 1)) - 1;
    r.bw = (hi & ((1 << kCubeMipFaceShift) - 1)) - 1 - r.c0 + 1;
    r.face = face;
    const bool one_face = face == (hi >> kCubeMipFaceShift);
    const bool in_range = r.r0 >= 0 && r.r0 + r.bh <= T && r.c0 >= 0 && r.c0 + r.bw <= T;
    if (one_face && in_range && (int64_t)r.bh * r.bw <= budget) {
        r.mode = kCubeMipBox;
        r.texels = (int64_t)r.bh * r.bw;
    }
    return r;
}

// One workgroup per 16 x 16 screen tile of one frame (blockIdx.x = (frame * tiles_y + tile_y) * tiles_x + tile_x).
template <int C>
__global__ __launch_bounds__(kLightThreads) void cubemap_sample_mip_bwd_kernel(
    const float *__restrict__ packed, int64_t frame_stride, int64_t n_face, int S, int L,
    const float *__restrict__ directions, const uint8_t *__restrict__ mask, const float *__restrict__ lod_in,
    float lod_bias, const float *__restrict__ lod_saved, int H, int W, int tiles_x, int tiles_y, int seamless,
    const float *__restrict__ grad, float *__restrict__ grad_packed, float *__restrict__ grad_directions,
    float *__restrict__ grad_lod)
{
    __shared__ float s_patch[(kCubeMipPatchTexels > 0 ? kCubeMipPatchTexels : 1) * C];
    __shared__ int s_box[9];  // the lowest k0; then per level A, B the four words of cube_mip_box_reduce

    const int tx = (int)(blockIdx.x % (unsigned)tiles_x);
    const int64_t rest = blockIdx.x / (unsigned)tiles_x;
    const int ty = (int)(rest % tiles_y);
    const int64_t frame = rest / tiles_y;
    const int y = ty * kTexTile + (int)(threadIdx.x / kTexTile), x = tx * kTexTile + (int)(threadIdx.x % kTexTile);
    const bool inside = y < H && x < W;
    const int64_t p = (frame * H + (inside ? y : 0)) * W + (inside ? x : 0);
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    const bool ok = inside && cube_sampled(directions, mask, p, &dx, &dy, &dz);
    const int64_t fbase = frame * frame_stride;
    const bool seam = seamless != 0;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = 0.0f;
    CubeCoord cc = {0, 1.0f, 1.0f, 0.0f, 0.0f, 0.5f, 0.5f};
    MipPick pk = mip_pick(0.0f, S, S, L);
    if (ok) {
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = grad[p * C + c];
        pk = mip_pick(lod_saved[p], S, S, L);
        cc = cube_coord(dx, dy, dz);
    }
    const bool two = ok && pk.f != 0.0f, above = ok && pk.k0 + 1 < L;  // (above: level k1 is not level k0)
    const float omf = 1.0f - pk.f;
    // (a lane that samples nothing takes the centre of face +x at level 0: in range, and never added or read)
    const CubeTaps t0 = cube_mip_taps(cc, pk.l0.w, seam), t1 = cube_mip_taps(cc, pk.l1.w, seam);

    if ((grad_directions || grad_lod) && inside) {
        float gx = 0.0f, gy = 0.0f, gz = 0.0f, gl = 0.0f;
        if (ok) {
            const float *chain = packed + fbase;
            float q[4 * C], s0[C], gu, gv;
            cube_mip_gather<C>(chain, n_face, pk.l0.off, t0, q);
            cube_mip_grad_uv<C>(q, pk.l0.w, t0, g, &gu, &gv);
            if (grad_lod && above) cube_mip_bilinear<C>(q, t0, s0);
            if (two || (grad_lod && above)) {
                cube_mip_gather<C>(chain, n_face, pk.l1.off, t1, q);
                if (two) {
                    float gu1, gv1;
                    cube_mip_grad_uv<C>(q, pk.l1.w, t1, g, &gu1, &gv1);
                    gu = gu * omf + gu1 * pk.f;
                    gv = gv * omf + gv1 * pk.f;
                }
                if (grad_lod && above) {
                    float s1[C];
                    cube_mip_bilinear<C>(q, t1, s1);
                    const float given = lod_in[p], biased = given + lod_bias;
                    const bool pass = given == given && biased >= 0.0f && biased <= (float)(L - 1);
                    float sum = 0.0f;
#pragma unroll
                    for (int c = 0; c < C; ++c) sum += g[c] * (s1[c] - s0[c]);  // (the first sum adds to +0: exact)
                    gl = pass ? sum : 0.0f;
                }
            }
            cube_grad_direction(cc, gu, gv, &gx, &gy, &gz);
        }
        if (grad_directions) {
            grad_directions[p * 3] = gx;
            grad_directions[p * 3 + 1] = gy;
            grad_directions[p * 3 + 2] = gz;
        }
        if (grad_lod) grad_lod[p] = gl;
    }
    if (!grad_packed) return;  // (uniform)

    float *gp = grad_packed + fbase;
    const float w0 = two ? omf : 1.0f;

    if (kCubeMipPatchTexels > 0) {
        if (threadIdx.x < 9) s_box[threadIdx.x] = kTexBoxEmpty;
        __syncthreads();
        const int kmin_w = wave_min(ok ? pk.k0 : kTexBoxEmpty);
        if ((threadIdx.x & 63) == 0) atomicMin(&s_box[0], kmin_w);
        __syncthreads();
        const int kA = s_box[0];
        if (kA == kTexBoxEmpty) return;  // no sampled pixel in the tile (uniform)
        // this lane's taps at level A and at level B
        const bool hasA = ok && pk.k0 == kA, firstB = ok && pk.k0 == kA + 1, hasB = firstB || (hasA && two);
        cube_mip_box_reduce(hasA, cc.face, t0, s_box + 1);
        cube_mip_box_reduce(hasB, cc.face, firstB ? t0 : t1, s_box + 5);
        __syncthreads();
        const MipLevel lA = mip_level(S, S, kA), lB = kA + 1 < L ? mip_next(lA) : lA;
        // A takes the budget first, B what A leaves
        const CubeMipPlan pA = cube_mip_plan(s_box + 1, lA.w, kCubeMipPatchTexels);
        const CubeMipPlan pB = cube_mip_plan(s_box + 5, lB.w, kCubeMipPatchTexels - pA.texels);  // (uniform, both)
        if (pA.mode != kCubeMipMemory || pB.mode != kCubeMipMemory) {
            const int eA = (int)pA.texels * C, eB = (int)pB.texels * C;
            for (int e = threadIdx.x; e < eA + eB; e += kLightThreads) s_patch[e] = 0.0f;
            __syncthreads();
            if (hasA) cube_mip_scatter<C>(pA.mode, s_patch, pA.r0, pA.c0, pA.bw, gp, n_face, lA, t0, g, w0);
            else if (firstB) cube_mip_scatter<C>(pB.mode, s_patch + eA, pB.r0, pB.c0, pB.bw, gp, n_face, lB, t0, g, w0);
            else if (ok) cube_mip_scatter<C>(kCubeMipMemory, nullptr, 0, 0, 0, gp, n_face, pk.l0, t0, g, w0);
            if (two) {
                if (hasA) cube_mip_scatter<C>(pB.mode, s_patch + eA, pB.r0, pB.c0, pB.bw, gp, n_face, lB, t1, g, pk.f);
                else cube_mip_scatter<C>(kCubeMipMemory, nullptr, 0, 0, 0, gp, n_face, pk.l1, t1, g, pk.f);
            }
            __syncthreads();
            // flush, both levels' parts in one pass over their eA + eB floats
            for (int e = threadIdx.x; e < eA + eB; e += kLightThreads) {
                const float s = s_patch[e];
                if (s == 0.0f) continue;
                const bool second = e >= eA;
                const CubeMipPlan &pl = second ? pB : pA;
                const MipLevel &lv = second ? lB : lA;
                const int el = second ? e - eA : e;
                if (pl.mode == kCubeMipWhole) {
                    const int per_face = lv.w * lv.w * C, face = el / per_face;
                    atomicAdd(gp + ((int64_t)face * n_face + lv.off) * C + (el - face * per_face), s);
                } else {
                    tex_flush_add<C>(s, el, pl.r0, pl.c0, pl.bw, gp + ((int64_t)pl.face * n_face + lv.off) * C, lv.w);
                }
            }
            return;
        }
    }
    if (ok) cube_mip_scatter<C>(kCubeMipMemory, nullptr, 0, 0, 0, gp, n_face, pk.l0, t0, g, w0);
    if (two) cube_mip_scatter<C>(kCubeMipMemory, nullptr, 0, 0, 0, gp, n_face, pk.l1, t1, g, pk.f);
}
