// dirt_raster.hip -- MI355X (gfx950) software rasteriser behind the C ABI of include/dirt_mi355x.h.
//
// CDNA4 has no graphics pipeline, so the reference's GL fixed-function raster
// (csrc/rasterise_egl.cpp:440-487 + the NVIDIA driver) becomes a compute pipeline of three launches:
//
//   K1 setup_kernel    (setup_kernel.h) one thread per (frame, face): fetch 3 clip vertices, project +
//                      snap (R1/R2), edge equations (R3), depth plane (R4), guard-band clipping (R5, rare
//                      slow path); writes 128-B setup records + 32-B FaceData; counts its (coarse tile,
//                      record) pairs in LDS, reserves its range of every touched coarse-tile slab with one
//                      returning device atomic per (workgroup, tile) and writes the 8-B bin entries there.
//                      Filler workgroups past the faces zero the caller's gradient accumulators.
//   K4 raster_kernel   (raster_kernel.h) one 256-thread workgroup per 16x16 tile (a wave per 8x8 block), in
//                      phases: fused_frame_setup (small scenes: no K1, the frame's records set up in LDS);
//                      first loads + launch_housekeeping (parity publish, deep-cull report, zero-fill of the
//                      gradient accumulators); the visibility pass -- bin filter of the coarse slab,
//                      stage_round (survivors into LDS with tile-relative exact 32-bit edge values),
//                      build_wave_list and the list walk, each lane keeping the min (depth24<<32 | face) key
//                      of its pixel (long lists depth-culled); resolve_record; write_uncovered (background) or
//                      the barycentrics (R6), write_gbuf_outputs, and shade_gouraud / a procedural program:
//                      coalesced [B,H,W,C] writes + the int32 g-buffer + neighbour-coverage bits.  This fuses
//                      the reference's upload_background + raster + second pass + download_pixels
//                      (csrc/rasterise_egl.cu:16-129, rasterise_egl.cpp:370-503) into one HBM pass.
//   K5 grad_kernel     (grad_kernel.h) backward: dL/dbackground, dL/dvertex_colors and the
//                      filter-based dL/dvertices (README.md:146-147) for the gradient contract of
//                      csrc/rasterise_grad_common.h:19-24.
//
// This file holds the shared device helpers, the workspace layout and its views, validation and the C ABI; the
// three kernels live in the headers named above, included into this one translation unit, each followed by its
// typed launcher (launch_setup / launch_raster / launch_grad): the one function that writes the kernel's <<<>>> and
// knows its parameter order.  The entry points here fill a RasterLaunch / GradLaunch by field name, pick the channel
// specialisation with with_channels() and the variant with an if-chain of launcher calls, the raster's by named
// mode flags (launch_raster<CC, kRasterFused | kRasterGbuf>(a)).

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <algorithm>

#include "../../include/dirt_mi355x.h"
#include "raster_rules.h"
#include "oceanic.h"
#include "hill.h"

using namespace dirt;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *msg)
{
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            char _b[256];                                                               \
            snprintf(_b, sizeof(_b), "%s failed: %s", #expr, hipGetErrorString(_e));    \
            return fail(DIRT_EHIP, _b);                                                 \
        }                                                                               \
    } while (0)

// ------------------------------------------------------------------------------------------------
// Optional per-kernel event timing (bench.py roofline); off by default, host-side only.
enum KernelId { K_SETUP = 0, K_RASTER, K_GRAD, K_COUNT };
const char *const kKernelNames[K_COUNT] = {"setup_kernel", "raster_kernel", "grad_kernel"};
struct Profiler {
    bool enabled = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[K_COUNT];
} g_prof;

struct ProfScope {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    int id;
    ProfScope(int id_, hipStream_t s_) : s(s_), id(id_)
    {
        if (!g_prof.enabled) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, s);
    }
    ~ProfScope()
    {
        if (!a) return;
        (void)hipEventRecord(b, s);
        g_prof.ev[id].emplace_back(a, b);
    }
};

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------
// Workspace layout.  saved = records [B][6F] (128 B) + FaceData [B][F] (32 B) + 4 neighbour-coverage
// bits per pixel: what the backward reads.  scratch = two sets of per-coarse-tile counts (alternating
// forwards: see kParP), a flag area, and the coarse bins: one fixed-capacity slab per (frame, coarse tile).
//
// Binning is two-level.  Coarse tiles (64x64 px, 128x128 above 4096 px) are binned by the setup kernel
// itself: each workgroup of 256 faces counts its (record, coarse tile) pairs in LDS, reserves its range
// of every touched slab with one returning device atomic per (workgroup, coarse tile), and writes the
// entries -- no separate count/scan/fill passes (a dependent kernel boundary costs ~1.7 us, and the
// fill pass had to re-read every record).  HBM is plentiful (288 GB), so the default slab holds as many
// entries as the frame has faces (+25 % for clipped sub-triangles): a tile overflows only under that
// budget or an explicit small bin_capacity, and an overflowed tile's raster workgroup then filters every
// record of the frame itself (slow, exact).  The fine 16x16-tile binning happens inside the raster
// kernel, in LDS.
struct Layout {
    int ntx, nty, ntiles;     // fine tiles per frame
    int cshift, csize;        // coarse tile edge = 1 << cshift pixels
    int nctx, ncty, ncoarse;  // coarse tiles per frame (<= kMaxCoarse)
    int64_t nrec;
    size_t saved_fdata, saved_cov, saved_total;  // (the records start `saved`)
    size_t off_count, off_flag, off_bins, scratch_total;
    int64_t bin_capacity;     // entries in all slabs
    uint32_t slab;            // entries per (frame, coarse tile) slab
};

constexpr int kMaxCoarse = 4096;   // LDS histogram size in setup
#ifndef DIRT_BIN_THREADS
#define DIRT_BIN_THREADS 256
#endif
constexpr int kBinThreads = DIRT_BIN_THREADS;
// entries (4 GiB of the 288 GB HBM) above which the default slab shrinks: B = 64 frames of 1024^2 and 20k faces
// (config 5 on one GPU) keep the full F + F/4 + 64 per slab, so a mesh crowded into a few coarse tiles does
// not send them to the overflow path (dirt_debug_bin_occupancy reports the fullest slab)
constexpr int64_t kDefaultBinBudget = 1ll << 29;
// Count-set parity, so that no kernel has to return the counts it read to zero.  Words of the flag area
// (separate 64-B lines): [0] out-of-range-face flag, [kParP] P, [kParQ] Q.  The setup kernel reads p = Q,
// publishes P = p, accumulates into counts[p] and zeroes counts[p ^ 1] (read by the previous forward's
// raster, which has completed); the raster kernel bins from counts[0] + counts[1] (= counts[p], the
// other set being zero) and publishes Q = P ^ 1 for the next forward.  Each word is only read by one kernel and only written (one workgroup,
// one value) by the other, so no launch reads a word it writes.  Zeroed scratch = a valid state.
constexpr int kParP = 16, kParQ = 32;
// Words between two bin counters: the setup's reservation atomics execute at the memory side, and ~200
// workgroups reserving in the same few lines serialise there, so every counter gets a line of its own.
#ifndef DIRT_COUNT_STRIDE
#define DIRT_COUNT_STRIDE 64
#endif
constexpr int kCountStride = DIRT_COUNT_STRIDE;

int64_t default_capacity(int B, int F, int ncoarse)
{
    const int64_t slabs = (int64_t)B * ncoarse;
    int64_t per = (int64_t)F + F / 4 + 64;
    if (slabs * per > kDefaultBinBudget) per = std::max<int64_t>(kDefaultBinBudget / std::max<int64_t>(slabs, 1), 256);
    return slabs * per;
}

int make_layout(int B, int H, int W, int F, int64_t bin_capacity, Layout &L)
{
    L.ntx = (W + kTile - 1) / kTile;
    L.nty = (H + kTile - 1) / kTile;
    L.ntiles = L.ntx * L.nty;
#ifndef DIRT_COARSE_SHIFT
#define DIRT_COARSE_SHIFT 6  // coarse tile edge 64 px (grown until the frame has <= kMaxCoarse of them)
#endif
    for (L.cshift = DIRT_COARSE_SHIFT;; ++L.cshift) {
        L.csize = 1 << L.cshift;
        L.nctx = (W + L.csize - 1) >> L.cshift;
        L.ncty = (H + L.csize - 1) >> L.cshift;
        L.ncoarse = L.nctx * L.ncty;
        if (L.ncoarse <= kMaxCoarse) break;
    }
    L.nrec = (int64_t)(1 + kExtraPerFace) * F;
    const int64_t slabs = std::max<int64_t>((int64_t)B * L.ncoarse, 1);
    L.bin_capacity = bin_capacity > 0 ? bin_capacity : default_capacity(B, F, L.ncoarse);
    L.slab = (uint32_t)std::min<int64_t>(std::max<int64_t>(L.bin_capacity / slabs, 1), 0x7fffffffLL);
    L.bin_capacity = (int64_t)L.slab * slabs;
    L.saved_fdata = (size_t)align_up((int64_t)B * L.nrec * (int64_t)sizeof(Rec), 256);
    L.saved_cov = L.saved_fdata + (size_t)align_up((int64_t)B * F * (int64_t)sizeof(FaceData), 256);
    L.saved_total = L.saved_cov + (size_t)align_up((int64_t)B * H * W, 256);  // 4 coverage bits per pixel
    const int64_t nc = (int64_t)B * L.ncoarse;
    size_t o = 0;
    L.off_count = o;  o += (size_t)align_up(2 * nc * 4 * kCountStride, 256);  // counts[2][B][ncoarse] (strided)
    L.off_flag = o;   o += 256;
    L.off_bins = o;   o += (size_t)align_up(L.bin_capacity * 8, 256);
    L.scratch_total = o;
    return DIRT_OK;
}

int validate(int B, int H, int W, int C, int V, int F)
{
    if (B < 0 || V < 0 || F < 0) return fail(DIRT_EINVAL, "Rasterise expects non-negative batch, vertex and face counts");
    if (H <= 0 || W <= 0 || H > DIRT_MAX_DIM || W > DIRT_MAX_DIM)
        return fail(DIRT_EINVAL, "Rasterise expects 0 < height, width <= 8192");
    if (C < 1 || C > DIRT_MAX_CHANNELS) return fail(DIRT_EINVAL, "Rasterise expects 1 <= channels <= 8");
    if (F > (1 << 26) || (int64_t)B * F > 0x0fffffffLL || (int64_t)B * V > 0x7fffffffLL)
        return fail(DIRT_EINVAL, "Rasterise batch too large (at most 2^26 faces per frame, 2^28 per batch)");
    return DIRT_OK;
}

// The arrays inside `saved` and `scratch`: Layout offsets applied to a base pointer (const: the readers of `saved`)
template <class T> T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(base) + off); }
template <class T> const T *at(const void *base, size_t off) { return at<T>(const_cast<void *>(base), off); }
struct SavedView {
    Rec *recs;
    FaceData *fdata;
    uint8_t *covbits;
    SavedView(const Layout &L, void *p)
        : recs(at<Rec>(p, 0)), fdata(at<FaceData>(p, L.saved_fdata)), covbits(at<uint8_t>(p, L.saved_cov)) {}
};
struct ConstSavedView {
    const Rec *recs;
    const FaceData *fdata;
    const uint8_t *covbits;
    ConstSavedView(const Layout &L, const void *p)
        : recs(at<Rec>(p, 0)), fdata(at<FaceData>(p, L.saved_fdata)), covbits(at<uint8_t>(p, L.saved_cov)) {}
};
struct ScratchView {
    uint32_t *ccount, *flag;
    uint2 *bins;
    ScratchView(const Layout &L, void *p)
        : ccount(at<uint32_t>(p, L.off_count)), flag(at<uint32_t>(p, L.off_flag)), bins(at<uint2>(p, L.off_bins)) {}
};

// The compile-time channel specialisation of a run-time C: 1, 3 and 7 have their own, every other count takes the
// generic one (CC = 0).  Calls fn(std::integral_constant<int, CC>{}).
template <class Fn>
void with_channels(int C, Fn &&fn)
{
    if (C == 1) fn(std::integral_constant<int, 1>{});
    else if (C == 3) fn(std::integral_constant<int, 3>{});
    else if (C == 7) fn(std::integral_constant<int, 7>{});
    else fn(std::integral_constant<int, 0>{});
}

// Every channel count its own specialisation (the deferred per-pixel ops: dilation, texture sampling): calls
// fn(std::integral_constant<int, C>{}) for the run-time C in 1..DIRT_MAX_CHANNELS, which the callers have validated.
template <class Fn>
void with_each_channel_count(int C, Fn &&fn)
{
    switch (C) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 3: fn(std::integral_constant<int, 3>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 5: fn(std::integral_constant<int, 5>{}); break;
    case 6: fn(std::integral_constant<int, 6>{}); break;
    case 7: fn(std::integral_constant<int, 7>{}); break;
    default: fn(std::integral_constant<int, 8>{}); break;
    }
}

// Start / stop events of a timed debug entry point, released on every path out of it.  (ProfScope's events outlive
// their scope on purpose: dirt_profile_read reads them later.)
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    hipError_t create()
    {
        const hipError_t e = hipEventCreate(&a);
        return e == hipSuccess ? hipEventCreate(&b) : e;
    }
    // create both events and record the first on `stream`
    hipError_t start(hipStream_t stream)
    {
        const hipError_t e = create();
        return e == hipSuccess ? hipEventRecord(a, s = stream) : e;
    }
    // record the second and wait for it; *ms = the time between the two
    hipError_t stop(float *ms)
    {
        hipError_t e = hipEventRecord(b, s);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        return e == hipSuccess ? hipEventElapsedTime(ms, a, b) : e;
    }
};

#include "setup_kernel.h"
#include "raster_kernel.h"
#include "grad_kernel.h"
#include "lighting_kernels.h"
#include "deferred_kernels.h"
#include "shade_lights_kernels.h"
#include "shade_pbr_kernels.h"
#include "shade_sh_kernels.h"
#include "shade_env_kernels.h"
#include "texture_kernels.h"
#include "cubemap_kernels.h"
#include "texture_mip_kernels.h"
#include "cubemap_mip_kernels.h"
#include "shadow_kernels.h"

// zero two float arrays in one launch (the backward's atomically accumulated outputs)
__global__ __launch_bounds__(256) void zero2_kernel(float *__restrict__ a, int64_t na, float *__restrict__ b, int64_t nb)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_strided(a, na, gid, stride);
    zero_strided(b, nb, gid, stride);
}

// PMC calibration (tools/pmc_calibrate.py): read `n` elements of W bytes once each, coalesced, with the
// access widths the product kernels use, so FETCH_SIZE can be converted to bytes per width
template <int W>
__global__ __launch_bounds__(256) void read_bytes_kernel(const char *__restrict__ src, int64_t n, float *out)
{
    float acc = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const char *p = src + e * W;
        if (W == 4) acc += *reinterpret_cast<const float *>(p);
        if (W == 12) {
            const float *q = reinterpret_cast<const float *>(p);
            acc += q[0] + q[1] + q[2];
        }
        if (W == 16) {
            const float4 q = *reinterpret_cast<const float4 *>(p);
            acc += q.x + q.y + q.z + q.w;
        }
    }
    if (acc == 1.2345e-30f) out[0] = acc;  // keep the loads
}

__global__ void check_faces_kernel(const int32_t *__restrict__ faces, int64_t n, int V, uint32_t *flag)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        if (faces[k] < 0 || faces[k] >= V) atomicOr(flag, 1u);
}

// ---- gradient stash of the single-output op (header words: setup_kernel.h kStash*)
struct StashDims {
    uint32_t d[5];  // B, H, W, V, F
};

// words of a and b equal?  (16-B loads when both are 16-B aligned, the tail and misaligned buffers by words)
__device__ __forceinline__ bool words_differ(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int64_t n,
                                             int64_t gid, int64_t gs)
{
    bool diff = false;
    const bool vec = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t k = gid; k < n4; k += gs) {
        const uint4 x = reinterpret_cast<const uint4 *>(a)[k], y = reinterpret_cast<const uint4 *>(b)[k];
        diff = diff || x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
    }
    for (int64_t k = 4 * n4 + gid; k < n; k += gs) diff = diff || a[k] != b[k];
    return diff;
}

// Does the workspace hold the records of exactly this geometry?  Bitwise comparison of vertices and faces with the
// copies the last forward-stash or recompute left (the records, g-buffer and coverage bits are a deterministic
// function of those bits and the frame size), plus the header's magic and dims.  Any difference sets this call's
// miss flag; the next call's flag is zeroed here (nothing reads it in this call).
__global__ __launch_bounds__(256) void stash_check_kernel(const uint32_t *__restrict__ v, const uint32_t *__restrict__ vt,
                                                          int64_t nv, const uint32_t *__restrict__ f,
                                                          const uint32_t *__restrict__ ft, int64_t nf, uint32_t *hdr,
                                                          StashDims dims)
{
    const uint32_t p = hdr[kStashP] & 1u;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (int64_t)gridDim.x * blockDim.x;
    bool miss = words_differ(v, vt, nv, gid, gs) || words_differ(f, ft, nf, gid, gs);
    if (gid == 0) {
        hdr[kStashMiss + 16 * (p ^ 1u)] = 0u;
        miss = miss || hdr[kStashMagicW] != kStashMagic;
        for (int k = 0; k < 5; ++k) miss = miss || hdr[kStashDims + k] != dims.d[k];
    }
    if (__ballot(miss) != 0 && (threadIdx.x & 63) == 0) atomicOr(&hdr[kStashMiss + 16 * p], 1u);
}

// zero n bytes (a multiple of 4, 4-B aligned) with a kernel: the scratch / stash clears run inside HIP graphs that
// the public op captures, and a kernel node is ordered like every other kernel of the graph
__global__ __launch_bounds__(256) void zero_words_kernel(uint32_t *__restrict__ p, int64_t n)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) p[k] = 0u;
}

__global__ void stash_flip_kernel(uint32_t *p)
{
    if (threadIdx.x == 0) p[0] ^= 1u;
}

// zero `bytes` (multiple of 4) at p on `stream` with zero_words_kernel
int zero_async(void *p, size_t bytes, hipStream_t stream)
{
    const int64_t n = (int64_t)(bytes / 4);
    if (n == 0) return DIRT_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(1024, (n + 255) / 256);
    zero_words_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(static_cast<uint32_t *>(p), n);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}


// After a recomputation (this call's miss flag set), or unconditionally for a forward-stash (`force`): record the
// geometry the workspace now holds.
__global__ __launch_bounds__(256) void stash_update_kernel(const uint32_t *__restrict__ v, uint32_t *__restrict__ vt,
                                                           int64_t nv, const uint32_t *__restrict__ f,
                                                           uint32_t *__restrict__ ft, int64_t nf, uint32_t *hdr,
                                                           StashDims dims, int force)
{
    if (!force && stash_hit(hdr)) return;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = gid; k < nv; k += gs) vt[k] = v[k];
    for (int64_t k = gid; k < nf; k += gs) ft[k] = f[k];
    if (gid == 0) {
        hdr[kStashMagicW] = kStashMagic;
        for (int k = 0; k < 5; ++k) hdr[kStashDims + k] = dims.d[k];
    }
}

}  // namespace

// ================================================================================================
// C ABI

extern "C" {

int dirt_abi_version(void) { return 13; }

const char *dirt_last_error(void) { return g_last_error.c_str(); }

int dirt_workspace_sizes(int B, int H, int W, int C, int V, int F, int64_t bin_capacity, size_t *saved_bytes,
                         size_t *scratch_bytes)
{
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    Layout L;
    rc = make_layout(B, H, W, F, bin_capacity, L);
    if (rc) return rc;
    if (saved_bytes) *saved_bytes = L.saved_total;
    if (scratch_bytes) *scratch_bytes = L.scratch_total;
    return DIRT_OK;
}

}  // extern "C"

// Automatic deep-scene culling: the Gouraud raster counts its long per-wave entry lists
// (raster_kernel deep_host) into one of two count slots of its scratch's flag area, and the next launch on the same
// scratch reports whether that count made the previous launch deep, by writing the previous launch's generation into
// a host-mapped word per device, then clears that slot.  A forward takes the occluder-culling instantiation (OCC)
// when a launch within the last kDeepRecent generations was deep: a deep scene switches after one launch (plus the
// queue's lag), a scene turning shallow switches back after kDeepRecent.  Both instantiations are exact, so the
// choice changes time only.  DIRT_FWD_DEEP_CULL forces OCC, DIRT_FWD_DEEP_CULL_OFF the plain raster;
// DIRT_DEEP_CULL_AUTO=0 disables the rule.
// Per scratch, the host remembers the generation and count slot of the last launch on it, so
// launches on several scratches interleaved on one device (two layouts, streams or sessions) each report their own
// previous launch; a launch counts into the slot its predecessor on that scratch did not use.  A launch captured
// into a graph neither counts nor reports (its instantiation is fixed at capture; replays would re-count into one
// slot forever), and the word is allocated outside any capture (relaxed capture mode, so another
// thread's global-mode capture is not invalidated by the host allocation).
constexpr uint32_t kDeepRecent = 8;
struct DeepScratch {
    const void *flag = nullptr;  // the scratch's flag area (identifies the scratch)
    uint32_t gen = 0;            // generation of the last launch on it
    uint32_t slot = 0;           // the count slot that launch used
};
constexpr int kDeepScratches = 64;
struct DeepAuto {
    uint32_t *host = nullptr;  // host-mapped word: generation of the last launch reported deep (0 = none)
    uint32_t *dev = nullptr;   // its device address
    uint32_t gen = 0;          // launches issued with the rule on
    DeepScratch scr[kDeepScratches];  // recently used scratches (round-robin replacement)
    int next = 0;
};
static std::mutex g_deep_mu;
static DeepAuto g_deep[64];

static bool deep_auto_enabled()
{
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("DIRT_DEEP_CULL_AUTO");
        v = (e && *e) ? (atoi(e) != 0) : 1;
    }
    return v != 0;
}

// the device's state with its word allocated (nullptr: rule off or the allocation failed)
static DeepAuto *deep_auto_state()
{
    if (!deep_auto_enabled()) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    DeepAuto &d = g_deep[dev];
    std::lock_guard<std::mutex> lk(g_deep_mu);
    if (d.host) return &d;
    // (relaxed capture mode for this thread: a host allocation is an unsafe call while any stream captures in
    // global mode, torch.cuda.graph's default)
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    void *h = nullptr, *dp = nullptr;
    bool ok = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    if (ok && hipHostGetDevicePointer(&dp, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        ok = false;
    }
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (!ok) return nullptr;
    static_cast<volatile uint32_t *>(h)[0] = 0u;
    d.dev = static_cast<uint32_t *>(dp);
    d.host = static_cast<uint32_t *>(h);
    return &d;
}

// the record of `flag`'s scratch (created on first use: no previous launch, generation 0); g_deep_mu held
static DeepScratch &deep_scratch(DeepAuto &d, const void *flag)
{
    for (DeepScratch &e : d.scr)
        if (e.flag == flag) return e;
    DeepScratch &e = d.scr[d.next];
    d.next = (d.next + 1) % kDeepScratches;
    e = DeepScratch{flag, 0u, 0u};
    return e;
}

// the forward of every op; tcb = channels of `background` (== C except for hill's terrain lookup)
static int rasterise_fwd_impl(const float *background, int tcb, const float *vertices, const float *vertex_colors,
                              const int32_t *faces, const float *camera_pos, int B, int H, int W, int C, int V, int F,
                              int shader_id, float *pixels, int32_t *gbuffer, void *saved, size_t saved_bytes,
                              void *scratch, size_t scratch_bytes, int64_t bin_capacity, unsigned flags,
                              float *zero_grad_vertices, float *zero_grad_vertex_colors, void *stream_,
                              GbufOut gbo = GbufOut{}, bool nopix = false, const uint32_t *stash_hdr = nullptr)
{
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    const bool want_gb = gbo.depth || gbo.bary || gbo.face;
    if (want_gb && shader_id != DIRT_SHADER_GOURAUD)
        return fail(DIRT_EINVAL, "Rasterise: depth / barycentric / face outputs are produced by the Gouraud program only");
    if (shader_id < DIRT_SHADER_GOURAUD || shader_id > DIRT_SHADER_HILL)
        return fail(DIRT_EINVAL, "Rasterise: unsupported shader_id");
    if (shader_id != DIRT_SHADER_GOURAUD && !camera_pos)
        return fail(DIRT_EINVAL, "Rasterise: procedural fragment programs need camera_pos");
    if (shader_id == DIRT_SHADER_HILL && tcb != 1 && tcb != 3 && tcb != 4)
        return fail(DIRT_EINVAL, "Hill: the terrain lookup must have 1, 3 or 4 channels");
    if (B == 0) return DIRT_OK;
    if (nopix && (shader_id != DIRT_SHADER_GOURAUD || want_gb))
        return fail(DIRT_EINVAL, "Rasterise: the coverage-only pass is Gouraud without G-buffer outputs");
    // (nopix: the coverage-only pass of dirt_rasterise_bwd_recompute reads no background or colours)
    const bool need_colors = shader_id == DIRT_SHADER_GOURAUD && !nopix;
    if ((!nopix && (!background || !pixels)) || !gbuffer || !saved || !scratch || (F > 0 && (!faces || !vertices)) ||
        (V > 0 && (!vertices || (need_colors && !vertex_colors))))
        return fail(DIRT_EINVAL, "Rasterise: null tensor pointer");
    Layout L;
    rc = make_layout(B, H, W, F, bin_capacity, L);
    if (rc) return rc;
    if (saved_bytes < L.saved_total || scratch_bytes < L.scratch_total)
        return fail(DIRT_EINVAL, "Rasterise: workspace smaller than dirt_workspace_sizes()");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const SavedView sv(L, saved);
    const ScratchView sc(L, scratch);

    // count sets and parity words: one memset, unless the caller vouches that the scratch is clean
    // (DIRT_FWD_SCRATCH_CLEAN: zeroed once and since used only by forwards of the same layout)
    if (!(flags & DIRT_FWD_SCRATCH_CLEAN)) {
        rc = zero_async(sc.ccount, L.off_bins - L.off_count, stream);
        if (rc) return rc;
    }
    // small scenes (Gouraud, F <= kFusedMaxF, at most kFusedMaxTiles tiles): the raster sets up the faces itself
    // (one launch, no bins)
    const bool fused = shader_id == DIRT_SHADER_GOURAUD && F > 0 && F <= kFusedMaxF &&
                       (int64_t)B * L.ntiles <= kFusedMaxTiles;
    // occluder culling of long per-wave entry lists (deep scenes, raster_kernel.h OCC): forced by DIRT_FWD_DEEP_CULL,
    // else automatic (DeepAuto) for the binned Gouraud forward
    bool deep = (flags & DIRT_FWD_DEEP_CULL) != 0 && shader_id == DIRT_SHADER_GOURAUD && !nopix;
    DeepArgs dga{};
    if (shader_id == DIRT_SHADER_GOURAUD && !nopix && !fused && !want_gb && F > 0 && !(flags & DIRT_FWD_DEEP_CULL_OFF)) {
        if (DeepAuto *da = deep_auto_state()) {
            // (a launch captured into a graph neither counts nor reports, nor does it advance the generation: it
            // does not execute now, and its replays keep the instantiation chosen here)
            hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
            const bool capturing = hipStreamIsCapturing(stream, &cst) == hipSuccess && cst != hipStreamCaptureStatusNone;
            std::lock_guard<std::mutex> lk(g_deep_mu);
            const uint32_t last = static_cast<volatile uint32_t *>(da->host)[0];
            const uint32_t next_gen = da->gen + 1u == 0u ? 1u : da->gen + 1u;  // (0 means "never deep")
            deep = deep || (last != 0u && next_gen - last <= kDeepRecent);
            if (!capturing) {
                da->gen = next_gen;
                DeepScratch &ds = deep_scratch(*da, sc.flag);
                dga.host = da->dev;
                dga.gen = next_gen;
                dga.prev_gen = ds.gen;
                dga.slot = ds.slot ^ 1u;
                ds.gen = next_gen;
                ds.slot = dga.slot;
            }
        }
    }
    if (F > 0 && !fused) {
        ProfScope ps(K_SETUP, stream);
        launch_setup<0>(vertices, faces, B, H, W, V, F, L, sv, sc, stream, zero_grad_vertices, (int64_t)B * V * 4,
                        zero_grad_vertex_colors, (int64_t)B * V * C, stash_hdr);
        HIP_TRY(hipGetLastError());
        // (the setup grid's filler workgroups zero the accumulators; the raster does it only when F == 0)
        zero_grad_vertices = nullptr;
        zero_grad_vertex_colors = nullptr;
    }
    ProfScope ps(K_RASTER, stream);
    // what every variant takes; the outputs and inputs of one variant alone are set in its branch below
    RasterLaunch a = raster_launch(L, B, H, W, C, V, F, stream);
    a.background = background; a.colors = vertex_colors; a.pixels = pixels; a.gbuffer = gbuffer;
    a.recs = sv.recs; a.fdata = sv.fdata; a.covbits = sv.covbits;
    a.counts = sc.ccount; a.flag = sc.flag; a.bins = sc.bins; a.slab = L.slab;
    a.zero_a = zero_grad_vertices; a.zero_b = zero_grad_vertex_colors;
    a.verts = vertices; a.cam = camera_pos; a.sid = shader_id; a.tcb = tcb;
    with_channels(C, [&](auto cc) {
        constexpr int CC = decltype(cc)::value;
        if (shader_id == DIRT_SHADER_OCEANIC_HORIZON) launch_raster<CC, 0, DIRT_SHADER_OCEANIC_HORIZON>(a);
        else if (shader_id == DIRT_SHADER_HILL) launch_raster<CC, 0, DIRT_SHADER_HILL>(a);
        else if (shader_id >= DIRT_SHADER_OCEANIC) launch_raster<CC, 0, DIRT_SHADER_OCEANIC>(a);
        else if (nopix && fused) {
            a.gbo = gbo; a.faces = faces; a.stash_hdr = stash_hdr;
            launch_raster<CC, kRasterFused | kRasterNoPix>(a);
        } else if (nopix) {
            a.gbo = gbo; a.stash_hdr = stash_hdr;
            launch_raster<CC, kRasterNoPix>(a);
        } else if (deep && !fused && !want_gb) {
            a.dga = dga;
            launch_raster<CC, kRasterOcc>(a);
        } else if (fused && want_gb) {
            a.gbo = gbo; a.faces = faces;
            launch_raster<CC, kRasterFused | kRasterGbuf>(a);
        } else if (fused) {
            a.gbo = gbo; a.faces = faces;
            launch_raster<CC, kRasterFused>(a);
        } else if (want_gb) {
            a.gbo = gbo;
            launch_raster<CC, kRasterGbuf>(a);
        } else {
            a.dga = dga;
            launch_raster<CC>(a);
        }
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

extern "C" {

int dirt_rasterise_fwd(const float *background, const float *vertices, const float *vertex_colors,
                       const int32_t *faces, const float *camera_pos, int B, int H, int W, int C, int V, int F,
                       int shader_id, float *pixels, int32_t *gbuffer, void *saved, size_t saved_bytes, void *scratch,
                       size_t scratch_bytes, int64_t bin_capacity, unsigned flags, float *zero_grad_vertices,
                       float *zero_grad_vertex_colors, void *stream_)
{
    return rasterise_fwd_impl(background, C, vertices, vertex_colors, faces, camera_pos, B, H, W, C, V, F, shader_id,
                              pixels, gbuffer, saved, saved_bytes, scratch, scratch_bytes, bin_capacity, flags,
                              zero_grad_vertices, zero_grad_vertex_colors, stream_);
}

int dirt_rasterise_fwd_gbuffer(const float *background, const float *vertices, const float *vertex_colors,
                               const int32_t *faces, int B, int H, int W, int C, int V, int F, float *pixels,
                               int32_t *gbuffer, void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes,
                               int64_t bin_capacity, unsigned flags, float *zero_grad_vertices,
                               float *zero_grad_vertex_colors, float *depth, float *barycentrics, int32_t *face_ids,
                               void *stream_)
{
    return rasterise_fwd_impl(background, C, vertices, vertex_colors, faces, nullptr, B, H, W, C, V, F,
                              DIRT_SHADER_GOURAUD, pixels, gbuffer, saved, saved_bytes, scratch, scratch_bytes,
                              bin_capacity, flags, zero_grad_vertices, zero_grad_vertex_colors, stream_,
                              GbufOut{depth, barycentrics, face_ids});
}

// A render sharing its geometry with the earlier Gouraud forward that filled gbuffer_in / saved (ABI 13): the resolve
// alone, over this render's colours and background (raster_kernel RESOLVE)
int dirt_rasterise_fwd_resolve(const float *background, const float *vertex_colors, int B, int H, int W, int C, int V,
                               int F, const int32_t *gbuffer_in, const void *saved, size_t saved_bytes, float *pixels,
                               int32_t *gbuffer, float *zero_grad_vertices, float *zero_grad_vertex_colors, void *stream_)
{
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    if (B == 0) return DIRT_OK;
    if (!background || !pixels || !gbuffer || !gbuffer_in || !saved || (V > 0 && !vertex_colors))
        return fail(DIRT_EINVAL, "RasteriseResolve: null tensor pointer");
    Layout L;
    rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    if (saved_bytes < L.saved_total) return fail(DIRT_EINVAL, "RasteriseResolve: saved smaller than dirt_workspace_sizes()");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ConstSavedView sv(L, saved);
    ProfScope ps(K_RASTER, stream);
    // (no bins, counts, coverage bits, vertices or camera: the visible record comes from gbuffer_in)
    RasterLaunch a = raster_launch(L, B, H, W, C, V, F, stream);
    a.background = background; a.colors = vertex_colors; a.pixels = pixels; a.gbuffer = gbuffer;
    a.recs = sv.recs; a.fdata = sv.fdata; a.gb_in = gbuffer_in;
    a.zero_a = zero_grad_vertices; a.zero_b = zero_grad_vertex_colors;
    with_channels(C, [&](auto cc) {
        launch_raster<decltype(cc)::value, kRasterResolve>(a);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_hill_fwd(const float *terrain, int terrain_channels, const float *vertices, const int32_t *faces,
                  const float *camera_pos, int B, int H, int W, int C, int V, int F, float *pixels, int32_t *gbuffer,
                  void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, int64_t bin_capacity,
                  void *stream_)
{
    return rasterise_fwd_impl(terrain, terrain_channels, vertices, nullptr, faces, camera_pos, B, H, W, C, V, F,
                              DIRT_SHADER_HILL, pixels, gbuffer, saved, saved_bytes, scratch, scratch_bytes,
                              bin_capacity, 0u, nullptr, nullptr, stream_);
}

}  // extern "C"

// dirt_debug_bwd_variant's ablation AB of the backward (C == 3 or 7, both gradients)
template <int AB>
static void launch_grad_3or7(const GradLaunch &g)
{
    if (g.C == 3) launch_grad<3, AB>(g);
    else launch_grad<7, AB>(g);
}

// the backward of dirt_rasterise_bwd; stash_flip: the recompute workspace's stash parity (flipped by the launch)
static int rasterise_bwd_impl(const float *vertices, const float *vertex_colors, const int32_t *faces,
                              const float *pixels, const float *grad_pixels, const int32_t *gbuffer, const void *saved,
                              int B, int H, int W, int C, int V, int F, float *grad_vertices, float *grad_vertex_colors,
                              float *grad_background, unsigned flags, void *stream_, uint32_t *stash_flip)
{
    // vertices / vertex_colors / faces are part of the contract (rasterise_grad_common.h:19-24); the
    // forward's FaceData in `saved` already holds what the kernel needs from them.
    (void)vertex_colors;
    (void)vertices;
    (void)faces;
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    if (B == 0) return DIRT_OK;
    if (!pixels || !grad_pixels || !gbuffer || !saved || (V > 0 && !grad_vertices && !grad_vertex_colors))
        return fail(DIRT_EINVAL, "RasteriseGrad: null tensor pointer");
    Layout L;
    rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    // which gradients to produce: a null grad_vertices / grad_vertex_colors is not computed at all (GM bits)
    const int gm = (grad_vertices ? 1 : 0) | (grad_vertex_colors ? 2 : 0);
    if (V > 0 && !(flags & DIRT_BWD_ACCUMULATE)) {
        const int64_t na = grad_vertices ? (int64_t)B * V * 4 : 0, nb = grad_vertex_colors ? (int64_t)B * V * C : 0;
        const int64_t blocks = std::min<int64_t>(2048, (std::max(na, nb) / 4 + 255) / 256 + 1);
        zero2_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(grad_vertices, na, grad_vertex_colors, nb);
        HIP_TRY(hipGetLastError());
    }
    if (gm == 0) {
        // V == 0 (no vertex or colour gradient exists): the launch still writes grad_background; the colour
        // path's instantiation with a null colour pointer has nothing to flush (every pixel is background)
        if (!grad_background) {
            if (stash_flip) {  // (no grad launch to flip the stash parity)
                stash_flip_kernel<<<dim3(1), dim3(64), 0, stream>>>(stash_flip);
                HIP_TRY(hipGetLastError());
            }
            return DIRT_OK;
        }
    }
    ProfScope ps(K_GRAD, stream);
    GradLaunch g = grad_launch(L, saved, B, H, W, C, V, F, stream);
    g.pixels = pixels; g.grad_pixels = grad_pixels; g.gbuffer = gbuffer;
    g.grad_verts = grad_vertices; g.grad_colors = grad_vertex_colors; g.grad_bg = grad_background;
    g.stash_flip = stash_flip;
    with_channels(C, [&](auto cc) {
        constexpr int CC = decltype(cc)::value;
        if (gm == 1) launch_grad<CC, 0, 1>(g);
        else if (gm == 2) launch_grad<CC, 0, 2>(g);
        else launch_grad<CC, 0, 3>(g);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

extern "C" {

int dirt_rasterise_bwd(const float *vertices, const float *vertex_colors, const int32_t *faces, const float *pixels,
                       const float *grad_pixels, const int32_t *gbuffer, const void *saved, int B, int H, int W, int C,
                       int V, int F, float *grad_vertices, float *grad_vertex_colors, float *grad_background,
                       unsigned flags, void *stream_)
{
    return rasterise_bwd_impl(vertices, vertex_colors, faces, pixels, grad_pixels, gbuffer, saved, B, H, W, C, V, F,
                              grad_vertices, grad_vertex_colors, grad_background, flags, stream_, nullptr);
}

// Workspace of the recompute backward: [saved | scratch | g-buffer | stash header | vertex copy | face copy], each
// 256-B aligned.  The stash (ABI v11): the geometry (vertices, faces, bitwise) whose records, g-buffer and coverage
// bits the workspace holds, written by dirt_rasterise_fwd_stash or after a recomputation.
struct RecomputeParts {
    size_t off_scratch, off_gbuf, off_hdr, off_vtag, off_ftag, total;
};
static RecomputeParts recompute_parts(const Layout &L, int B, int H, int W, int V, int F)
{
    RecomputeParts P;
    P.off_scratch = (size_t)align_up((int64_t)L.saved_total, 256);
    P.off_gbuf = P.off_scratch + (size_t)align_up((int64_t)L.scratch_total, 256);
    P.off_hdr = P.off_gbuf + (size_t)align_up((int64_t)B * H * W * 4, 256);
    P.off_vtag = P.off_hdr + 256;
    P.off_ftag = P.off_vtag + (size_t)align_up((int64_t)B * V * 16, 256);
    P.total = P.off_ftag + (size_t)align_up((int64_t)B * F * 12, 256);
    return P;
}

// launch the stash check (check = true) or update of a recompute workspace for this geometry
static int launch_stash(bool check, bool force, const float *vertices, const int32_t *faces, int B, int H, int W,
                        int V, int F, char *ws, const RecomputeParts &P, hipStream_t stream)
{
    const int64_t nv = (int64_t)B * V * 4, nf = (int64_t)B * F * 3;
    const StashDims dims{{(uint32_t)B, (uint32_t)H, (uint32_t)W, (uint32_t)V, (uint32_t)F}};
    uint32_t *hdr = reinterpret_cast<uint32_t *>(ws + P.off_hdr);
    uint32_t *vt = reinterpret_cast<uint32_t *>(ws + P.off_vtag), *ft = reinterpret_cast<uint32_t *>(ws + P.off_ftag);
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (std::max(nv / 4, nf) + 255) / 256));
    if (check)
        stash_check_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(reinterpret_cast<const uint32_t *>(vertices), vt, nv,
                                                                   reinterpret_cast<const uint32_t *>(faces), ft, nf,
                                                                   hdr, dims);
    else
        stash_update_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(reinterpret_cast<const uint32_t *>(vertices), vt,
                                                                    nv, reinterpret_cast<const uint32_t *>(faces), ft,
                                                                    nf, hdr, dims, force ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_bwd_recompute_workspace_size(int B, int H, int W, int C, int V, int F, size_t *workspace_bytes)
{
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    Layout L;
    rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    if (workspace_bytes) *workspace_bytes = recompute_parts(L, B, H, W, V, F).total;
    return DIRT_OK;
}

// The registered gradient of the single-output op: upstream DIRT's gradient re-derived its G-buffer from the
// op's inputs (csrc/rasterise_grad_common.h:5-24: launch_vertex_upload, then launch_grad_assembly on pixels,
// grad_pixels and vertices).  Here: setup + binning + a coverage-only raster pass (g-buffer and the
// neighbour-coverage bits, bit-identical to the forward's: same integer rules, same inputs) into the
// caller's workspace, then the same backward kernel as dirt_rasterise_bwd.
int dirt_rasterise_bwd_recompute(const float *background, const float *vertices, const float *vertex_colors,
                                 const int32_t *faces, const float *pixels, const float *grad_pixels, int B, int H,
                                 int W, int C, int V, int F, float *grad_vertices, float *grad_vertex_colors,
                                 float *grad_background, void *workspace, size_t workspace_bytes, unsigned flags,
                                 void *stream_)
{
    (void)background;  // part of the op's inputs (the gradient of an uncovered pixel does not depend on it)
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    if (B == 0) return DIRT_OK;
    if (!pixels || !grad_pixels || !workspace || (F > 0 && (!faces || !vertices)) ||
        (V > 0 && !grad_vertices && !grad_vertex_colors))
        return fail(DIRT_EINVAL, "RasteriseGrad: null tensor pointer");
    Layout L;
    rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    const RecomputeParts P = recompute_parts(L, B, H, W, V, F);
    if (workspace_bytes < P.total)
        return fail(DIRT_EINVAL, "RasteriseGrad: workspace smaller than dirt_bwd_recompute_workspace_size()");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    char *ws = static_cast<char *>(workspace);
    int32_t *gbuf = reinterpret_cast<int32_t *>(ws + P.off_gbuf);
    uint32_t *hdr = reinterpret_cast<uint32_t *>(ws + P.off_hdr);
    const bool acc = (flags & DIRT_BWD_ACCUMULATE) != 0;
    const bool clean = (flags & DIRT_BWD_SCRATCH_CLEAN) != 0;
    // (a workspace not vouched clean starts from scratch: bin counters and the stash header zeroed -- a miss)
    if (!clean) {
        rc = zero_async(hdr, 256, stream);
        if (rc) return rc;
    }
    // stash check: does the workspace already hold this geometry's records, g-buffer and coverage bits (left by
    // dirt_rasterise_fwd_stash or by the previous recomputation)?  The recomputation below then exits at once
    // (device-side; the setup's filler workgroups still zero the accumulators).
    rc = launch_stash(true, false, vertices, faces, B, H, W, V, F, ws, P, stream);
    if (rc) return rc;
    // the recomputation zero-fills the gradient accumulators in passing (setup filler workgroups), so the
    // backward below only adds into them
    rc = rasterise_fwd_impl(nullptr, C, vertices, nullptr, faces, nullptr, B, H, W, C, V, F, DIRT_SHADER_GOURAUD,
                            nullptr, gbuf, ws, L.saved_total, ws + P.off_scratch, L.scratch_total, 0,
                            clean ? DIRT_FWD_SCRATCH_CLEAN : 0u, acc ? nullptr : grad_vertices,
                            acc ? nullptr : grad_vertex_colors, stream_, GbufOut{}, /*nopix=*/true, hdr);
    if (rc) return rc;
    // after a recomputation the workspace holds this geometry: record it for the next call
    rc = launch_stash(false, false, vertices, faces, B, H, W, V, F, ws, P, stream);
    if (rc) return rc;
    return rasterise_bwd_impl(vertices, vertex_colors, faces, pixels, grad_pixels, gbuf, ws, B, H, W, C, V, F,
                              grad_vertices, grad_vertex_colors, grad_background, DIRT_BWD_ACCUMULATE, stream_, hdr);
}

// The single-output op's forward with its gradient stash: dirt_rasterise_fwd (Gouraud) whose records, g-buffer and
// coverage bits go into a recompute workspace, which then also records the geometry; a dirt_rasterise_bwd_recompute
// with that workspace and bitwise the same vertices and faces skips its recomputation.
int dirt_rasterise_fwd_stash(const float *background, const float *vertices, const float *vertex_colors,
                             const int32_t *faces, int B, int H, int W, int C, int V, int F, float *pixels,
                             void *workspace, size_t workspace_bytes, unsigned flags, void *stream_)
{
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    if (B == 0) return DIRT_OK;
    if (!workspace) return fail(DIRT_EINVAL, "Rasterise: null workspace");
    Layout L;
    rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    const RecomputeParts P = recompute_parts(L, B, H, W, V, F);
    if (workspace_bytes < P.total)
        return fail(DIRT_EINVAL, "Rasterise: workspace smaller than dirt_bwd_recompute_workspace_size()");
    char *ws = static_cast<char *>(workspace);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const bool clean = (flags & DIRT_FWD_SCRATCH_CLEAN) != 0;
    if (!clean) {
        rc = zero_async(ws + P.off_hdr, 256, stream);
        if (rc) return rc;
    }
    rc = rasterise_fwd_impl(background, C, vertices, vertex_colors, faces, nullptr, B, H, W, C, V, F,
                            DIRT_SHADER_GOURAUD, pixels, reinterpret_cast<int32_t *>(ws + P.off_gbuf), ws,
                            L.saved_total, ws + P.off_scratch, L.scratch_total, 0, clean ? DIRT_FWD_SCRATCH_CLEAN : 0u,
                            nullptr, nullptr, stream_);
    if (rc) return rc;
    return launch_stash(false, true, vertices, faces, B, H, W, V, F, ws, P, stream);
}

__global__ void bin_occupancy_kernel(const uint32_t *__restrict__ counts, int64_t nslabs, uint32_t slab, uint32_t *out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nslabs; k += (int64_t)gridDim.x * blockDim.x) {
        // this forward's count set holds the counts, the other set is zero (kParP)
        const uint32_t n = counts[k * kCountStride] + counts[(nslabs + k) * kCountStride];
        atomicMax(&out[0], n);
        if (n > slab) atomicAdd(&out[1], 1u);
    }
}

// Debug (synchronises `stream`): the bin occupancy the last forward left in `scratch` -- the fullest slab's
// entry count, the number of slabs that overflowed (their tiles took the all-records path) and the slab
// capacity.  Not part of include/dirt_mi355x.h.
int dirt_debug_bin_occupancy(int B, int H, int W, int F, int64_t bin_capacity, const void *scratch,
                             size_t scratch_bytes, void *stream_, uint32_t *max_count, uint32_t *overflowed,
                             uint32_t *slab)
{
    Layout L;
    int rc = make_layout(B, H, W, F, bin_capacity, L);
    if (rc) return rc;
    if (!scratch || scratch_bytes < L.scratch_total) return fail(DIRT_EINVAL, "dirt_debug_bin_occupancy: scratch too small");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    uint32_t *d = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&d), 8, stream));
    HIP_TRY(hipMemsetAsync(d, 0, 8, stream));
    const int64_t nslabs = (int64_t)B * L.ncoarse;
    bin_occupancy_kernel<<<dim3(256), dim3(256), 0, stream>>>(
        reinterpret_cast<const uint32_t *>(static_cast<const char *>(scratch) + L.off_count), nslabs, L.slab, d);
    HIP_TRY(hipGetLastError());
    uint32_t h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipFreeAsync(d, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (max_count) *max_count = h[0];
    if (overflowed) *overflowed = h[1];
    if (slab) *slab = L.slab;
    return DIRT_OK;
}

// Debug: the current device's hipDeviceAttributeMaxGridDimY, or 0 where it cannot be read.  The batch B is grid.y of
// the setup, raster, grad and vertex-normal launches; launches beyond the attribute's 65536 run on an MI355X
// (tests/test_gpu_large_frames.py renders 65537 frames, tests/test_gpu_lighting_f64.py 70,000), so nothing is
// refused by it.  Not part of include/dirt_mi355x.h.
int dirt_debug_max_grid_y(void)
{
    int dev = 0, lim = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxGridDimY, dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return lim;
}

// Debug (synchronises `stream`): the R5 deviation counters of `scratch` (setup_kernel.h kStatCapCulled /
// kStatClamped), summed over every forward since the scratch was last cleared: faces culled by the R5 vertex cap
// and clipped faces whose sub-vertices the R5 clamp moved.  reset != 0 zeroes them afterwards.  Not part of
// include/dirt_mi355x.h.
int dirt_debug_clip_stats(int B, int H, int W, int F, int64_t bin_capacity, void *scratch, size_t scratch_bytes,
                          void *stream_, int reset, uint32_t *cap_culled, uint32_t *clamped)
{
    Layout L;
    int rc = make_layout(B, H, W, F, bin_capacity, L);
    if (rc) return rc;
    if (!scratch || scratch_bytes < L.scratch_total) return fail(DIRT_EINVAL, "dirt_debug_clip_stats: scratch too small");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    uint32_t *flag = ScratchView(L, scratch).flag;
    uint32_t h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&h[0], flag + kStatCapCulled, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&h[1], flag + kStatClamped, 4, hipMemcpyDeviceToHost, stream));
    if (reset) {
        HIP_TRY(hipMemsetAsync(flag + kStatCapCulled, 0, 4, stream));
        HIP_TRY(hipMemsetAsync(flag + kStatClamped, 0, 4, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (cap_culled) *cap_culled = h[0];
    if (clamped) *clamped = h[1];
    return DIRT_OK;
}

// Debug (host only, no GPU call): the workspace layout of these dimensions and the constants a reader of `saved` and
// `scratch` needs, as int64 words in the order below (dirt_amd/_lib.py LAYOUT_FIELDS names them); writes the
// first n and returns EINVAL when n exceeds their number.  Not part of include/dirt_mi355x.h.
int dirt_debug_layout(int B, int H, int W, int F, int64_t bin_capacity, int64_t *out, int n)
{
    Layout L;
    int rc = make_layout(B, H, W, F, bin_capacity, L);
    if (rc) return rc;
    const int64_t v[] = {
        L.cshift, L.nctx, L.ncty, (int64_t)L.slab, L.nrec,
        (int64_t)L.saved_fdata, (int64_t)L.saved_cov, (int64_t)L.saved_total,
        (int64_t)L.off_count, (int64_t)L.off_flag, (int64_t)L.off_bins, (int64_t)L.scratch_total,
        kCountStride, kParP, kParQ, kStatCapCulled, kStatClamped,
        (int64_t)sizeof(Rec), (int64_t)sizeof(FaceData), kRecBboxOffset,
        kFusedMaxF, kFusedMaxTiles, kSmallPairs, kBigCap, kBinThreads, kSetupSmallGrid,
    };
    const int nv = (int)(sizeof(v) / sizeof(v[0]));
    if (!out || n < 0 || n > nv) return fail(DIRT_EINVAL, "dirt_debug_layout: out null or n out of range");
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return DIRT_OK;
}

// Debug: the automatic deep-cull rule of the current device (DeepAuto): launches issued with it, the generation of
// the last launch reported deep (0 = none), and whether the next forward would take the occluder instantiation.
// Not part of include/dirt_mi355x.h.
int dirt_debug_deep_cull_state(uint32_t *gen, uint32_t *last_deep, int *next_deep)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(DIRT_EINVAL, "dirt_debug_deep_cull_state: device index");
    std::lock_guard<std::mutex> lk(g_deep_mu);
    const DeepAuto &d = g_deep[dev];
    const uint32_t last = d.host ? static_cast<volatile uint32_t *>(d.host)[0] : 0u;
    if (gen) *gen = d.gen;
    if (last_deep) *last_deep = last;
    if (next_deep) *next_deep = (last != 0u && d.gen + 1u - last <= kDeepRecent) ? 1 : 0;
    return DIRT_OK;
}

// Debug (synchronises `stream`): whether the last dirt_rasterise_bwd_recompute on `workspace` recomputed (1: the
// stash did not hold its geometry) or reused the stash (0), and the header's magic word.  Not part of
// include/dirt_mi355x.h.
int dirt_debug_stash_state(int B, int H, int W, int C, int V, int F, const void *workspace, size_t workspace_bytes,
                           void *stream_, uint32_t *last_missed, uint32_t *magic)
{
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    Layout L;
    rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    const RecomputeParts P = recompute_parts(L, B, H, W, V, F);
    if (!workspace || workspace_bytes < P.total) return fail(DIRT_EINVAL, "dirt_debug_stash_state: workspace too small");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    uint32_t h[64];
    HIP_TRY(hipMemcpyAsync(h, static_cast<const char *>(workspace) + P.off_hdr, 256, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t p = h[kStashP] & 1u;  // (the last call's grad launch flipped it: that call used p ^ 1)
    if (last_missed) *last_missed = h[kStashMiss + 16 * (p ^ 1u)];
    if (magic) *magic = h[kStashMagicW];
    return DIRT_OK;
}

// Ablation entry point (tools/ablate.py): re-runs raster_kernel (C == 3) on the bins a preceding
// dirt_rasterise_fwd left in `scratch`, with parts switched off; returns the kernel time in ms.
int dirt_debug_raster_variant(int variant, const float *background, const float *vertices, const float *vertex_colors,
                              const int32_t *faces, int B, int H, int W, int C, int V, int F, float *pixels,
                              int32_t *gbuffer, void *saved, void *scratch, void *stream_, float *ms)
{
    if (C != 3) return fail(DIRT_EINVAL, "dirt_debug_raster_variant: C must be 3");
    Layout L;
    int rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const SavedView sv(L, saved);
    const ScratchView sc(L, scratch);
    // re-bin from a clean scratch, then time the raster variant alone
    HIP_TRY(hipMemsetAsync(sc.ccount, 0, L.off_bins - L.off_count, stream));
    if (F > 0) launch_setup<0>(vertices, faces, B, H, W, V, F, L, sv, sc, stream);
    RasterLaunch a = raster_launch(L, B, H, W, C, V, F, stream);
    a.background = background; a.colors = vertex_colors; a.pixels = pixels; a.gbuffer = gbuffer;
    a.recs = sv.recs; a.fdata = sv.fdata; a.covbits = sv.covbits;
    a.counts = sc.ccount; a.flag = sc.flag; a.bins = sc.bins; a.slab = L.slab;
    EventPair ev;
    HIP_TRY(ev.start(stream));
    constexpr int G = DIRT_SHADER_GOURAUD;  // (the ablation mask AB is the launcher's last parameter)
    switch (variant) {
    case 0: launch_raster<3, 0, G, 0>(a); break;        case 1: launch_raster<3, 0, G, 1>(a); break;
    case 2: launch_raster<3, 0, G, 2>(a); break;        case 4: launch_raster<3, 0, G, 4>(a); break;
    case 8: launch_raster<3, 0, G, 8>(a); break;        case 32: launch_raster<3, 0, G, 32>(a); break;
    case 64: launch_raster<3, 0, G, 64>(a); break;      case 96: launch_raster<3, 0, G, 96>(a); break;
    case 128: launch_raster<3, 0, G, 128>(a); break;    case 512: launch_raster<3, 0, G, 512>(a); break;
    case 1024: launch_raster<3, 0, G, 1024>(a); break;  case 2048: launch_raster<3, 0, G, 2048>(a); break;
    default:
        return fail(DIRT_EINVAL, "dirt_debug_raster_variant: unknown variant");
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(ev.stop(ms));
    return DIRT_OK;
}

// Instrumented setup (tools/setup_ts.py): clean scratch, one setup_kernel<128> launch, its time in ms;
// per-workgroup phase timestamps land in g_phase_ts (dirt_debug_read_phase_ts).
// variant 0: timestamps, 1: timestamps without the slab reservation atomics, 2 / 3: the same untimestamped
int dirt_debug_setup_ts(int variant, const float *vertices, const int32_t *faces, int B, int H, int W, int V, int F,
                        void *saved, void *scratch, void *stream_, float *ms)
{
    Layout L;
    int rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const SavedView sv(L, saved);
    const ScratchView sc(L, scratch);
    HIP_TRY(hipMemsetAsync(sc.ccount, 0, L.off_bins - L.off_count, stream));
    EventPair ev;
    HIP_TRY(ev.start(stream));
    // variant -> setup_kernel's AB
    auto run = [&](auto ab) { launch_setup<decltype(ab)::value>(vertices, faces, B, H, W, V, F, L, sv, sc, stream); };
    switch (variant) {
    case 0: run(std::integral_constant<int, 128>{}); break;  case 1: run(std::integral_constant<int, 129>{}); break;
    case 2: run(std::integral_constant<int, 0>{}); break;    case 3: run(std::integral_constant<int, 1>{}); break;
    case 4: run(std::integral_constant<int, 2>{}); break;    case 5: run(std::integral_constant<int, 3>{}); break;
    case 6: run(std::integral_constant<int, 4>{}); break;
    default:
        return fail(DIRT_EINVAL, "dirt_debug_setup_ts: unknown variant");
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(ev.stop(ms));
    return DIRT_OK;
}

// Ablation entry point (tools/ablate.py): the backward with parts of grad_kernel switched off.
// Not part of include/dirt_mi355x.h; C == 3 or 7.  Returns the kernel time in ms (hipEvents).
int dirt_debug_bwd_variant(int variant, const float *pixels, const float *grad_pixels, const int32_t *gbuffer,
                           const void *saved, int B, int H, int W, int C, int V, int F, float *grad_vertices,
                           float *grad_vertex_colors, float *grad_background, void *stream_, float *ms)
{
    if (C != 3 && C != 7) return fail(DIRT_EINVAL, "dirt_debug_bwd_variant: C must be 3 or 7");
    Layout L;
    int rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    HIP_TRY(hipMemsetAsync(grad_vertices, 0, (size_t)B * V * 4 * sizeof(float), stream));
    HIP_TRY(hipMemsetAsync(grad_vertex_colors, 0, (size_t)B * V * C * sizeof(float), stream));
    GradLaunch g = grad_launch(L, saved, B, H, W, C, V, F, stream);
    g.pixels = pixels; g.grad_pixels = grad_pixels; g.gbuffer = gbuffer;
    g.grad_verts = grad_vertices; g.grad_colors = grad_vertex_colors; g.grad_bg = grad_background;
    EventPair ev;
    HIP_TRY(ev.start(stream));
    switch (variant) {
    case 0: launch_grad_3or7<0>(g); break;      case 1: launch_grad_3or7<1>(g); break;
    case 2: launch_grad_3or7<2>(g); break;      case 3: launch_grad_3or7<3>(g); break;
    case 4: launch_grad_3or7<4>(g); break;      case 5: launch_grad_3or7<5>(g); break;
    case 7: launch_grad_3or7<7>(g); break;      case 8: launch_grad_3or7<8>(g); break;
    case 16: launch_grad_3or7<16>(g); break;    case 32: launch_grad_3or7<32>(g); break;
    case 64: launch_grad_3or7<64>(g); break;    case 72: launch_grad_3or7<72>(g); break;
    case 128: launch_grad_3or7<128>(g); break;  case 256: launch_grad_3or7<256>(g); break;
    default:
        return fail(DIRT_EINVAL, "dirt_debug_bwd_variant: unknown variant");
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(ev.stop(ms));
    return DIRT_OK;
}

// Debug (synchronises `stream`): the product backward kernel (C == 3, vertex and colour gradients) launched `reps`
// times through hipExtLaunchKernel with start / stop events, which the runtime takes from the dispatch itself: the mean
// kernel duration in ms, as rocprofv3 --kernel-trace reports it (an event pair around an ordinary launch, or a graph of
// back-to-back launches, adds each launch's dependent-launch gap).  Accumulates into the gradient buffers.  bench.py's
// roofline uses it.  Not part of include/dirt_mi355x.h.
int dirt_debug_bwd_dispatch_ms(const float *pixels, const float *grad_pixels, const int32_t *gbuffer, const void *saved,
                               int B, int H, int W, int C, int V, int F, float *grad_vertices, float *grad_vertex_colors,
                               float *grad_background, int reps, void *stream_, float *ms)
{
    if (C != 3 || !grad_vertices || !grad_vertex_colors || reps < 1 || !ms)
        return fail(DIRT_EINVAL, "dirt_debug_bwd_dispatch_ms: C == 3, both gradient buffers, reps >= 1");
    int rc = validate(B, H, W, C, V, F);
    if (rc) return rc;
    if (!pixels || !grad_pixels || !gbuffer || !saved) return fail(DIRT_EINVAL, "dirt_debug_bwd_dispatch_ms: null pointer");
    Layout L;
    rc = make_layout(B, H, W, F, 0, L);
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GradLaunch g = grad_launch(L, saved, B, H, W, C, V, F, stream);
    g.pixels = pixels; g.grad_pixels = grad_pixels; g.gbuffer = gbuffer;
    g.grad_verts = grad_vertices; g.grad_colors = grad_vertex_colors; g.grad_bg = grad_background;
    EventPair ev;
    hipError_t err = ev.create();
    float total = 0.0f;
    for (int r = 0; r < reps && err == hipSuccess; ++r) {
        launch_grad<3, 0, 3>(g, ev.a, ev.b);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipEventSynchronize(ev.b);
        float t = 0.0f;
        if (err == hipSuccess) err = hipEventElapsedTime(&t, ev.a, ev.b);
        total += t;
    }
    HIP_TRY(err);
    *ms = total / (float)reps;
    return DIRT_OK;
}

int dirt_debug_read_bytes(int width, const void *src, size_t bytes, float *out, void *stream_)
{
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (width != 4 && width != 12 && width != 16) return fail(DIRT_EINVAL, "dirt_debug_read_bytes: width 4, 12 or 16");
    const int64_t n = (int64_t)(bytes / (size_t)width);
    const dim3 grid(2048), block(256);
    if (width == 4) read_bytes_kernel<4><<<grid, block, 0, stream>>>(static_cast<const char *>(src), n, out);
    if (width == 12) read_bytes_kernel<12><<<grid, block, 0, stream>>>(static_cast<const char *>(src), n, out);
    if (width == 16) read_bytes_kernel<16><<<grid, block, 0, stream>>>(static_cast<const char *>(src), n, out);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

// copy the phase timestamps of the last instrumented backward (variant 128): 10 words per workgroup (8 timestamps, HW_ID, XCC_ID)
int dirt_debug_read_phase_ts(uint64_t *host, int nwg)
{
    if (nwg < 0 || nwg > kTsMaxWG) return fail(DIRT_EINVAL, "dirt_debug_read_phase_ts: bad count");
    HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_phase_ts), (size_t)nwg * kTsStride * sizeof(uint64_t), 0,
                                hipMemcpyDeviceToHost));
    return DIRT_OK;
}

int dirt_profile_enable(int enable)
{
    for (int k = 0; k < K_COUNT; ++k) {
        for (auto &p : g_prof.ev[k]) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        g_prof.ev[k].clear();
    }
    g_prof.enabled = enable != 0;
    return DIRT_OK;
}

int dirt_profile_read(int kernel_id, const char **name, int *launches, double *total_ms)
{
    if (kernel_id < 0 || kernel_id >= K_COUNT) return fail(DIRT_EINVAL, "dirt_profile_read: bad kernel id");
    double tot = 0.0;
    for (auto &p : g_prof.ev[kernel_id]) {
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        tot += ms;
    }
    if (name) *name = kKernelNames[kernel_id];
    if (launches) *launches = (int)g_prof.ev[kernel_id].size();
    if (total_ms) *total_ms = tot;
    return DIRT_OK;
}

int dirt_scratch_clear(int B, int H, int W, int F, int64_t bin_capacity, void *scratch, size_t scratch_bytes,
                       void *stream_)
{
    if (B < 0 || F < 0 || H <= 0 || W <= 0 || H > DIRT_MAX_DIM || W > DIRT_MAX_DIM)
        return fail(DIRT_EINVAL, "dirt_scratch_clear: bad sizes");
    if (B == 0) return DIRT_OK;
    Layout L;
    const int rc = make_layout(B, H, W, F, bin_capacity, L);
    if (rc) return rc;
    if (!scratch || scratch_bytes < L.scratch_total)
        return fail(DIRT_EINVAL, "dirt_scratch_clear: scratch smaller than dirt_workspace_sizes()");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    return zero_async(static_cast<char *>(scratch) + L.off_count, L.off_bins - L.off_count, stream);
}

int dirt_stream_capture_id(void *stream_, unsigned long long *capture_id)
{
    if (!capture_id) return fail(DIRT_EINVAL, "dirt_stream_capture_id: null pointer");
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    HIP_TRY(hipStreamGetCaptureInfo(reinterpret_cast<hipStream_t>(stream_), &st, &id));
    *capture_id = st == hipStreamCaptureStatusActive ? id : 0ull;
    return DIRT_OK;
}

int dirt_check_faces(const int32_t *faces, int B, int V, int F, void *scratch, size_t scratch_bytes, void *stream_)
{
    if (B < 0 || F < 0 || V < 0) return fail(DIRT_EINVAL, "dirt_check_faces: negative size");
    if (!scratch || scratch_bytes < 256) return fail(DIRT_EINVAL, "dirt_check_faces: scratch too small");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    uint32_t *flag = reinterpret_cast<uint32_t *>(scratch);
    HIP_TRY(hipMemsetAsync(flag, 0, 4, stream));
    const int64_t n = (int64_t)B * F * 3;
    if (n > 0) {
        check_faces_kernel<<<dim3(1024), dim3(256), 0, stream>>>(faces, n, V, flag);
        HIP_TRY(hipGetLastError());
    }
    uint32_t h = 0;
    HIP_TRY(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h) return fail(DIRT_EFACE, "Rasterise: face index out of range [0, vertex count)");
    return DIRT_OK;
}


// ---- fused lighting helpers (lighting_kernels.h; dirt/lighting.py)

int dirt_vertex_normals_fwd(const float *vertices, int vertex_stride, const void *faces, int faces_int64, int B, int V,
                            int F, float *summed, float *normals, void *stream_)
{
    if (B < 0 || V < 0 || F < 0 || vertex_stride < 3)
        return fail(DIRT_EINVAL, "vertex_normals: negative size or vertex stride < 3");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t nv = (int64_t)B * V;
    if (nv == 0) return DIRT_OK;
    if (!vertices || !summed || !normals || (F > 0 && !faces)) return fail(DIRT_EINVAL, "vertex_normals: null pointer");
    int rc_z;
    rc_z = zero_async(summed, (size_t)nv * 3 * sizeof(float), stream);  // (a kernel: graph-captured like the rest)
    if (rc_z) return rc_z;
    if (F > 0 && B > 0) {
        const dim3 grid(light_blocks(F), (unsigned)B);
        if (faces_int64)
            vnormals_face_kernel<int64_t><<<grid, dim3(kLightThreads), 0, stream>>>(
                vertices, vertex_stride, static_cast<const int64_t *>(faces), V, F, summed);
        else
            vnormals_face_kernel<int32_t><<<grid, dim3(kLightThreads), 0, stream>>>(
                vertices, vertex_stride, static_cast<const int32_t *>(faces), V, F, summed);
        HIP_TRY(hipGetLastError());
    }
    vnormals_vertex_kernel<<<dim3(light_blocks(nv)), dim3(kLightThreads), 0, stream>>>(summed, nv, normals);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_vertex_normals_bwd(const float *vertices, int vertex_stride, const void *faces, int faces_int64, int B, int V,
                            int F, const float *summed, const float *grad_normals, float *grad_summed,
                            float *grad_vertices, int grad_stride, void *stream_)
{
    if (B < 0 || V < 0 || F < 0 || vertex_stride < 3 || grad_stride < 3)
        return fail(DIRT_EINVAL, "vertex_normals: negative size or vertex stride < 3");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t nv = (int64_t)B * V;
    if (nv == 0) return DIRT_OK;
    if (!vertices || !summed || !grad_normals || !grad_summed || !grad_vertices || (F > 0 && !faces))
        return fail(DIRT_EINVAL, "vertex_normals: null pointer");
    const int rc_z = zero_async(grad_vertices, (size_t)nv * grad_stride * sizeof(float), stream);
    if (rc_z) return rc_z;
    if (F == 0) return DIRT_OK;
    vnormals_vertex_bwd_kernel<<<dim3(light_blocks(nv)), dim3(kLightThreads), 0, stream>>>(summed, grad_normals, nv,
                                                                                          grad_summed);
    HIP_TRY(hipGetLastError());
    const dim3 grid(light_blocks(F), (unsigned)B);
    if (faces_int64)
        vnormals_face_bwd_kernel<int64_t><<<grid, dim3(kLightThreads), 0, stream>>>(
            vertices, vertex_stride, static_cast<const int64_t *>(faces), V, F, grad_summed, grad_vertices, grad_stride);
    else
        vnormals_face_bwd_kernel<int32_t><<<grid, dim3(kLightThreads), 0, stream>>>(
            vertices, vertex_stride, static_cast<const int32_t *>(faces), V, F, grad_summed, grad_vertices, grad_stride);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_diffuse_directional_fwd(const float *normals, const float *colors, int64_t N, const float *light_direction,
                                 const float *light_color, int double_sided, float *out, void *stream_)
{
    if (N < 0) return fail(DIRT_EINVAL, "diffuse_directional: negative size");
    if (N == 0) return DIRT_OK;
    if (!normals || !colors || !light_direction || !light_color || !out)
        return fail(DIRT_EINVAL, "diffuse_directional: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    diffuse_fwd_kernel<<<dim3(light_blocks(N)), dim3(kLightThreads), 0, stream>>>(normals, colors, N, light_direction,
                                                                                  light_color, double_sided, out);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_diffuse_directional_bwd(const float *normals, const float *colors, int64_t N, const float *light_direction,
                                 const float *light_color, int double_sided, const float *grad_out,
                                 float *grad_normals, float *grad_colors, void *stream_)
{
    if (N < 0) return fail(DIRT_EINVAL, "diffuse_directional: negative size");
    if (N == 0 || (!grad_normals && !grad_colors)) return DIRT_OK;
    if (!normals || !colors || !light_direction || !light_color || !grad_out)
        return fail(DIRT_EINVAL, "diffuse_directional: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    diffuse_bwd_kernel<<<dim3(light_blocks(N)), dim3(kLightThreads), 0, stream>>>(
        normals, colors, N, light_direction, light_color, double_sided, grad_out, grad_normals, grad_colors);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_diffuse_point_fwd(const float *positions, const float *normals, const float *colors, int64_t N,
                           const float *light_position, const float *light_color, int double_sided, float *out,
                           void *stream_)
{
    if (N < 0) return fail(DIRT_EINVAL, "diffuse_point: negative size");
    if (N == 0) return DIRT_OK;
    if (!positions || !normals || !colors || !light_position || !light_color || !out)
        return fail(DIRT_EINVAL, "diffuse_point: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    diffuse_point_fwd_kernel<<<dim3(light_blocks(N)), dim3(kLightThreads), 0, stream>>>(
        positions, normals, colors, N, light_position, light_color, double_sided, out);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_diffuse_point_bwd(const float *positions, const float *normals, const float *colors, int64_t N,
                           const float *light_position, const float *light_color, int double_sided,
                           const float *grad_out, float *grad_positions, float *grad_normals, float *grad_colors,
                           void *stream_)
{
    if (N < 0) return fail(DIRT_EINVAL, "diffuse_point: negative size");
    if (N == 0 || (!grad_positions && !grad_normals && !grad_colors)) return DIRT_OK;
    if (!positions || !normals || !colors || !light_position || !light_color || !grad_out)
        return fail(DIRT_EINVAL, "diffuse_point: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    diffuse_point_bwd_kernel<<<dim3(light_blocks(N)), dim3(kLightThreads), 0, stream>>>(
        positions, normals, colors, N, light_position, light_color, double_sided, grad_out, grad_positions,
        grad_normals, grad_colors);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_specular_directional_fwd(const float *positions, const float *normals, const float *reflectivities, int64_t N,
                                  const float *light_direction, const float *light_color,
                                  const float *camera_position, float shininess, int double_sided, float *out,
                                  void *stream_)
{
    if (N < 0) return fail(DIRT_EINVAL, "specular_directional: negative size");
    if (N == 0) return DIRT_OK;
    if (!positions || !normals || !reflectivities || !light_direction || !light_color || !camera_position || !out)
        return fail(DIRT_EINVAL, "specular_directional: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    specular_fwd_kernel<<<dim3(light_blocks(N)), dim3(kLightThreads), 0, stream>>>(
        positions, normals, reflectivities, N, light_direction, light_color, camera_position, shininess, double_sided,
        out);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_specular_directional_bwd(const float *positions, const float *normals, const float *reflectivities, int64_t N,
                                  const float *light_direction, const float *light_color,
                                  const float *camera_position, float shininess, int double_sided,
                                  const float *grad_out, float *grad_positions, float *grad_normals,
                                  float *grad_reflectivities, void *stream_)
{
    if (N < 0) return fail(DIRT_EINVAL, "specular_directional: negative size");
    if (N == 0 || (!grad_positions && !grad_normals && !grad_reflectivities)) return DIRT_OK;
    if (!positions || !normals || !reflectivities || !light_direction || !light_color || !camera_position || !grad_out)
        return fail(DIRT_EINVAL, "specular_directional: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    specular_bwd_kernel<<<dim3(light_blocks(N)), dim3(kLightThreads), 0, stream>>>(
        positions, normals, reflectivities, N, light_direction, light_color, camera_position, shininess, double_sided,
        grad_out, grad_positions, grad_normals, grad_reflectivities);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- deferred shading: silhouette dilation and the fused G-buffer lighting (deferred_kernels.h)

namespace {

// shared argument checks of the four entry points: DIRT_OK with *pixels = B * H * W (0: nothing to do)
int deferred_sizes(const char *op, int B, int H, int W, int C, int64_t *pixels)
{
    char msg[160];
    *pixels = 0;
    if (B < 0) {
        snprintf(msg, sizeof(msg), "%s: batch size must be non-negative", op);
        return fail(DIRT_EINVAL, msg);
    }
    if (H < 1 || W < 1 || H > DIRT_MAX_DIM || W > DIRT_MAX_DIM) {
        snprintf(msg, sizeof(msg), "%s: height, width must be in 1..%d", op, DIRT_MAX_DIM);
        return fail(DIRT_EINVAL, msg);
    }
    if (C < 1 || C > DIRT_MAX_CHANNELS) {
        snprintf(msg, sizeof(msg), "%s: expects 1 <= channels <= %d", op, DIRT_MAX_CHANNELS);
        return fail(DIRT_EINVAL, msg);
    }
    const int64_t n = (int64_t)B * H * W;
    if ((n + kLightThreads - 1) / kLightThreads > 0x7fffffffLL) {
        snprintf(msg, sizeof(msg), "%s: too large (more pixels than one launch covers)", op);
        return fail(DIRT_EINVAL, msg);
    }
    *pixels = n;
    return DIRT_OK;
}

template <int C>
void launch_dilate_fwd(const float *x, const uint8_t *mask, int H, int W, int64_t n, float *out, uint32_t *route,
                       hipStream_t stream)
{
    dilate_fwd_kernel<C><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(x, mask, H, W, n, out, route);
}

template <int C>
void launch_dilate_bwd(const float *grad, const uint32_t *route, int H, int W, int64_t n, float *grad_x,
                       hipStream_t stream)
{
    dilate_bwd_kernel<C><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(grad, route, H, W, n, grad_x);
}

ShadeLights shade_lights_of(const float *ambient_color, const float *light_direction, const float *diffuse_color,
                            const float *specular_color, const float *camera_position, float shininess, int double_sided)
{
    return {ambient_color, light_direction, diffuse_color, specular_color, camera_position, shininess, double_sided};
}

}  // namespace

extern "C" {

int dirt_dilate_fwd(const float *x, const uint8_t *mask, int B, int H, int W, int C, float *out, uint32_t *route,
                    void *stream_)
{
    int64_t n;
    const int rc = deferred_sizes("dilate", B, H, W, C, &n);
    if (rc || n == 0) return rc;
    if (!x || !out || !route) return fail(DIRT_EINVAL, "dilate: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    with_each_channel_count(C, [&](auto c) {
        launch_dilate_fwd<decltype(c)::value>(x, mask, H, W, n, out, route, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_dilate_bwd(const float *grad_out, const uint32_t *route, int B, int H, int W, int C, float *grad_x,
                    void *stream_)
{
    int64_t n;
    const int rc = deferred_sizes("dilate", B, H, W, C, &n);
    if (rc || n == 0) return rc;
    if (!grad_out || !route || !grad_x) return fail(DIRT_EINVAL, "dilate: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    with_each_channel_count(C, [&](auto c) {
        launch_dilate_bwd<decltype(c)::value>(grad_out, route, H, W, n, grad_x, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_shade_fwd(const float *positions, const float *colors, const float *normals, int B, int H, int W,
                            const float *ambient_color, const float *light_direction, const float *diffuse_color,
                            const float *specular_color, const float *camera_position, float shininess,
                            int double_sided, float *pixels, uint8_t *valid, uint32_t *route, void *stream_)
{
    int64_t n;
    const int rc = deferred_sizes("deferred_shade", B, H, W, 3, &n);
    if (rc || n == 0) return rc;
    if (!positions || !colors || !normals || !ambient_color || !light_direction || !diffuse_color || !specular_color ||
        !camera_position || !pixels || !valid || !route)
        return fail(DIRT_EINVAL, "deferred_shade: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeLights L = shade_lights_of(ambient_color, light_direction, diffuse_color, specular_color,
                                          camera_position, shininess, double_sided);
    deferred_shade_fwd_kernel<<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        positions, colors, normals, H, W, n, L, pixels, valid, route);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_shade_bwd(const float *positions, const float *colors, const float *normals, int B, int H, int W,
                            const float *ambient_color, const float *light_direction, const float *diffuse_color,
                            const float *specular_color, const float *camera_position, float shininess,
                            int double_sided, const float *grad_pixels, const uint32_t *route, float *grad_positions,
                            float *grad_colors, float *grad_normals, void *stream_)
{
    int64_t n;
    const int rc = deferred_sizes("deferred_shade", B, H, W, 3, &n);
    if (rc || n == 0 || (!grad_positions && !grad_colors && !grad_normals)) return rc;
    if (!positions || !colors || !normals || !ambient_color || !light_direction || !diffuse_color || !specular_color ||
        !camera_position || !grad_pixels || !route)
        return fail(DIRT_EINVAL, "deferred_shade: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeLights L = shade_lights_of(ambient_color, light_direction, diffuse_color, specular_color,
                                          camera_position, shininess, double_sided);
    deferred_shade_bwd_kernel<<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        positions, colors, normals, H, W, n, L, grad_pixels, route, grad_positions, grad_colors, grad_normals);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- deferred shading with many lights and gradients to them (shade_lights_kernels.h)

namespace {

// the argument checks the three entry points share beyond deferred_sizes': DIRT_OK with *pixels = B * H * W
int shade_lights_sizes(int B, int H, int W, int n_lights, unsigned point_mask, int64_t *pixels)
{
    const int rc = deferred_sizes("deferred_shade_lights", B, H, W, 3, pixels);
    if (rc) return rc;
    if (n_lights < 0 || n_lights > DIRT_MAX_LIGHTS) {
        char msg[160];
        snprintf(msg, sizeof(msg), "deferred_shade_lights: expects 0 <= lights <= %d", DIRT_MAX_LIGHTS);
        return fail(DIRT_EINVAL, msg);
    }
    if (point_mask >> n_lights) return fail(DIRT_EINVAL, "deferred_shade_lights: point_mask has bits past the lights");
    return DIRT_OK;
}

ShadeLightsArgs shade_lights_args(const float *ambient_color, int n_lights, unsigned point_mask, int lights_per_frame,
                                  const float *light_vectors, const float *diffuse_colors,
                                  const float *specular_colors, int camera_per_frame, const float *camera_position,
                                  float shininess_value, const float *shininess_ptr, int double_sided)
{
    return {ambient_color, light_vectors, diffuse_colors, specular_colors, camera_position, shininess_ptr,
            shininess_value, n_lights, point_mask, lights_per_frame != 0, camera_per_frame != 0, double_sided};
}

int64_t shade_lights_chunks(int H, int W) { return ((int64_t)H * W + kSlChunk - 1) / kSlChunk; }

size_t shade_lights_workspace_bytes(int B, int H, int W, int n_lights)
{
    return (size_t)B * (size_t)shade_lights_chunks(H, W) * (size_t)(kSlFixedSums + kSlSumsPerLight * n_lights) *
           sizeof(float);
}

}  // namespace

extern "C" {

int dirt_deferred_shade_lights_workspace(int B, int H, int W, int n_lights, size_t *bytes)
{
    int64_t n;
    const int rc = shade_lights_sizes(B, H, W, n_lights, 0u, &n);
    if (rc) return rc;
    if (!bytes) return fail(DIRT_EINVAL, "deferred_shade_lights: null pointer");
    *bytes = shade_lights_workspace_bytes(B, H, W, n_lights);
    return DIRT_OK;
}

int dirt_deferred_shade_lights_fwd(const float *positions, const float *colors, const float *normals, int B, int H,
                                   int W, const float *ambient_color, int n_lights, unsigned point_mask,
                                   int lights_per_frame, const float *light_vectors, const float *diffuse_colors,
                                   const float *specular_colors, int camera_per_frame, const float *camera_position,
                                   float shininess_value, const float *shininess_ptr, int double_sided, float *pixels,
                                   uint8_t *valid, uint32_t *route, void *stream_)
{
    int64_t n;
    const int rc = shade_lights_sizes(B, H, W, n_lights, point_mask, &n);
    if (rc || n == 0) return rc;
    if (!positions || !colors || !normals || !pixels || !valid || !route ||
        (n_lights > 0 && (!light_vectors || !diffuse_colors || !specular_colors || !camera_position)))
        return fail(DIRT_EINVAL, "deferred_shade_lights: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeLightsArgs A = shade_lights_args(ambient_color, n_lights, point_mask, lights_per_frame, light_vectors,
                                                diffuse_colors, specular_colors, camera_per_frame, camera_position,
                                                shininess_value, shininess_ptr, double_sided);
    shade_lights_fwd_kernel<<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        positions, colors, normals, H, W, n, A, pixels, valid, route);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_shade_lights_bwd(const float *positions, const float *colors, const float *normals, int B, int H,
                                   int W, const float *ambient_color, int n_lights, unsigned point_mask,
                                   int lights_per_frame, const float *light_vectors, const float *diffuse_colors,
                                   const float *specular_colors, int camera_per_frame, const float *camera_position,
                                   float shininess_value, const float *shininess_ptr, int double_sided,
                                   const float *grad_pixels, const uint32_t *route, float *grad_positions,
                                   float *grad_colors, float *grad_normals, float *grad_ambient,
                                   float *grad_light_vectors, float *grad_diffuse_colors, float *grad_specular_colors,
                                   float *grad_camera, float *grad_shininess, void *workspace, size_t workspace_bytes,
                                   void *stream_)
{
    int64_t n;
    const int rc = shade_lights_sizes(B, H, W, n_lights, point_mask, &n);
    if (rc || n == 0) return rc;
    if (n_lights == 0) grad_light_vectors = grad_diffuse_colors = grad_specular_colors = nullptr;  // (empty arrays)
    const bool want_params = grad_ambient || grad_light_vectors || grad_diffuse_colors || grad_specular_colors ||
                             grad_camera || grad_shininess;
    if (!want_params && !grad_positions && !grad_colors && !grad_normals) return DIRT_OK;
    if (!positions || !colors || !normals || !grad_pixels || !route ||
        (n_lights > 0 && (!light_vectors || !diffuse_colors || !specular_colors || !camera_position)))
        return fail(DIRT_EINVAL, "deferred_shade_lights: null pointer");
    if (want_params && (!workspace || workspace_bytes < shade_lights_workspace_bytes(B, H, W, n_lights)))
        return fail(DIRT_EINVAL, "deferred_shade_lights: workspace smaller than "
                                 "dirt_deferred_shade_lights_workspace() reports");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeLightsArgs A = shade_lights_args(ambient_color, n_lights, point_mask, lights_per_frame, light_vectors,
                                                diffuse_colors, specular_colors, camera_per_frame, camera_position,
                                                shininess_value, shininess_ptr, double_sided);
    const int chunks = (int)shade_lights_chunks(H, W);  // (at most 8192^2 / 1024)
    const dim3 grid((unsigned)chunks, (unsigned)std::min(B, 65535));
    float *partial = static_cast<float *>(workspace);
    if (want_params) {
        shade_lights_bwd_kernel<true><<<grid, dim3(kSlThreads), 0, stream>>>(
            positions, colors, normals, B, H, W, A, grad_pixels, route, grad_positions, grad_colors, grad_normals,
            partial);
        // the camera without lights, and the shininess without lights, receive exact zeros from the empty sums
        const SlParamGrads G = {grad_ambient, grad_light_vectors, grad_diffuse_colors, grad_specular_colors,
                                grad_camera, grad_shininess};
        shade_lights_reduce_kernel<<<dim3((unsigned)(kSlFixedSums + kSlSumsPerLight * n_lights)), dim3(kSlThreads), 0,
                                     stream>>>(partial, B, chunks, n_lights, lights_per_frame != 0,
                                               camera_per_frame != 0, G);
    } else {
        shade_lights_bwd_kernel<false><<<grid, dim3(kSlThreads), 0, stream>>>(
            positions, colors, normals, B, H, W, A, grad_pixels, route, grad_positions, grad_colors, grad_normals,
            nullptr);
    }
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- metallic-roughness deferred shading with gradients to everything (shade_pbr_kernels.h)

namespace {

// the argument checks the three entry points share beyond deferred_sizes': DIRT_OK with *pixels = B * H * W
int shade_pbr_sizes(int B, int H, int W, int n_lights, unsigned point_mask, int64_t *pixels)
{
    const int rc = deferred_sizes("deferred_shade_pbr", B, H, W, 3, pixels);
    if (rc) return rc;
    if (n_lights < 0 || n_lights > DIRT_MAX_LIGHTS) {
        char msg[160];
        snprintf(msg, sizeof(msg), "deferred_shade_pbr: expects 0 <= lights <= %d", DIRT_MAX_LIGHTS);
        return fail(DIRT_EINVAL, msg);
    }
    if (point_mask >> n_lights) return fail(DIRT_EINVAL, "deferred_shade_pbr: point_mask has bits past the lights");
    return DIRT_OK;
}

ShadePbrArgs shade_pbr_args(const float *ambient_color, int n_lights, unsigned point_mask, int lights_per_frame,
                            const float *light_vectors, const float *light_colors, int camera_per_frame,
                            const float *camera_position)
{
    return {ambient_color, light_vectors, light_colors, camera_position, n_lights, point_mask, lights_per_frame != 0,
            camera_per_frame != 0};
}

int64_t shade_pbr_chunks(int H, int W) { return ((int64_t)H * W + kSlThreads - 1) / kSlThreads; }

size_t shade_pbr_workspace_bytes(int B, int H, int W, int n_lights)
{
    return (size_t)B * (size_t)shade_pbr_chunks(H, W) * (size_t)(kPbrFixedSums + kPbrSumsPerLight * n_lights) *
           sizeof(float);
}

void launch_shade_pbr_fwd(const float *positions, const float *colors, const float *normals, const float *material,
                          const float *visibility, int H, int W, int64_t n, const ShadePbrArgs &A, float *pixels,
                          uint8_t *valid, uint32_t *route, hipStream_t stream)
{
    shade_pbr_fwd_kernel<<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        positions, colors, normals, material, visibility, H, W, n, A, pixels, valid, route);
}

template <bool kParams>
void launch_shade_pbr_bwd(const float *positions, const float *colors, const float *normals, const float *material,
                          const float *visibility, int B, int H, int W, const ShadePbrArgs &A, const float *grad_pixels,
                          const uint32_t *route, float *grad_positions, float *grad_colors, float *grad_normals,
                          float *grad_material, float *grad_visibility, float *partial, hipStream_t stream)
{
    const dim3 grid((unsigned)shade_pbr_chunks(H, W), (unsigned)std::min(B, 65535));  // (at most 8192^2 / 256 chunks)
    shade_pbr_bwd_kernel<kParams><<<grid, dim3(kSlThreads), 0, stream>>>(
        positions, colors, normals, material, visibility, B, H, W, A, grad_pixels, route, grad_positions, grad_colors,
        grad_normals, grad_material, grad_visibility, partial);
}

void launch_shade_pbr_reduce(const float *partial, int B, int chunks, int n_lights, int lights_per_frame,
                             int camera_per_frame, const PbrParamGrads &G, hipStream_t stream)
{
    shade_pbr_reduce_kernel<<<dim3((unsigned)(kPbrFixedSums + kPbrSumsPerLight * n_lights)), dim3(kSlThreads), 0,
                              stream>>>(partial, B, chunks, n_lights, lights_per_frame != 0, camera_per_frame != 0, G);
}

}  // namespace

extern "C" {

int dirt_deferred_shade_pbr_workspace(int B, int H, int W, int n_lights, size_t *bytes)
{
    int64_t n;
    const int rc = shade_pbr_sizes(B, H, W, n_lights, 0u, &n);
    if (rc) return rc;
    if (!bytes) return fail(DIRT_EINVAL, "deferred_shade_pbr: null pointer");
    *bytes = shade_pbr_workspace_bytes(B, H, W, n_lights);
    return DIRT_OK;
}

int dirt_deferred_shade_pbr_fwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *visibility, int B, int H, int W,
                                const float *ambient_color, int n_lights, unsigned point_mask, int lights_per_frame,
                                const float *light_vectors, const float *light_colors, int camera_per_frame,
                                const float *camera_position, float *pixels, uint8_t *valid, uint32_t *route,
                                void *stream_)
{
    int64_t n;
    const int rc = shade_pbr_sizes(B, H, W, n_lights, point_mask, &n);
    if (rc || n == 0) return rc;
    if (!positions || !colors || !normals || !material || !pixels || !valid || !route ||
        (n_lights > 0 && (!light_vectors || !light_colors || !camera_position)))
        return fail(DIRT_EINVAL, "deferred_shade_pbr: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadePbrArgs A = shade_pbr_args(ambient_color, n_lights, point_mask, lights_per_frame, light_vectors,
                                          light_colors, camera_per_frame, camera_position);
    launch_shade_pbr_fwd(positions, colors, normals, material, visibility, H, W, n, A, pixels, valid, route, stream);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_shade_pbr_bwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *visibility, int B, int H, int W,
                                const float *ambient_color, int n_lights, unsigned point_mask, int lights_per_frame,
                                const float *light_vectors, const float *light_colors, int camera_per_frame,
                                const float *camera_position, const float *grad_pixels, const uint32_t *route,
                                float *grad_positions, float *grad_colors, float *grad_normals, float *grad_material,
                                float *grad_visibility, float *grad_ambient, float *grad_light_vectors,
                                float *grad_light_colors, float *grad_camera, void *workspace, size_t workspace_bytes,
                                void *stream_)
{
    int64_t n;
    const int rc = shade_pbr_sizes(B, H, W, n_lights, point_mask, &n);
    if (rc || n == 0) return rc;
    if (n_lights == 0) grad_light_vectors = grad_light_colors = grad_visibility = nullptr;  // (empty arrays)
    const bool want_params = grad_ambient || grad_light_vectors || grad_light_colors || grad_camera;
    if (!want_params && !grad_positions && !grad_colors && !grad_normals && !grad_material && !grad_visibility)
        return DIRT_OK;
    if (!positions || !colors || !normals || !material || !grad_pixels || !route ||
        (n_lights > 0 && (!light_vectors || !light_colors || !camera_position)))
        return fail(DIRT_EINVAL, "deferred_shade_pbr: null pointer");
    if (want_params && (!workspace || workspace_bytes < shade_pbr_workspace_bytes(B, H, W, n_lights)))
        return fail(DIRT_EINVAL, "deferred_shade_pbr: workspace smaller than "
                                 "dirt_deferred_shade_pbr_workspace() reports");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadePbrArgs A = shade_pbr_args(ambient_color, n_lights, point_mask, lights_per_frame, light_vectors,
                                          light_colors, camera_per_frame, camera_position);
    float *partial = static_cast<float *>(workspace);
    if (want_params) {
        launch_shade_pbr_bwd<true>(positions, colors, normals, material, visibility, B, H, W, A, grad_pixels, route,
                                   grad_positions, grad_colors, grad_normals, grad_material, grad_visibility, partial,
                                   stream);
        // (the camera without lights receives exact zeros from the empty sums)
        const PbrParamGrads G = {grad_ambient, grad_light_vectors, grad_light_colors, grad_camera};
        launch_shade_pbr_reduce(partial, B, (int)shade_pbr_chunks(H, W), n_lights, lights_per_frame,
                                camera_per_frame, G, stream);
    } else {
        launch_shade_pbr_bwd<false>(positions, colors, normals, material, visibility, B, H, W, A, grad_pixels, route,
                                    grad_positions, grad_colors, grad_normals, grad_material, grad_visibility, nullptr,
                                    stream);
    }
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- deferred shading under spherical-harmonic lighting (shade_sh_kernels.h)

namespace {

// the argument checks the three entry points share beyond deferred_sizes': DIRT_OK with *pixels = B * H * W
int shade_sh_sizes(int B, int H, int W, int n_coeffs, int64_t *pixels)
{
    const int rc = deferred_sizes("deferred_shade_sh", B, H, W, 3, pixels);
    if (rc) return rc;
    if (n_coeffs != 1 && n_coeffs != 4 && n_coeffs != 9)
        return fail(DIRT_EINVAL, "deferred_shade_sh: expects 1, 4 or 9 coefficients (bands 0, 0-1, 0-2)");
    return DIRT_OK;
}

int64_t shade_sh_chunks(int H, int W) { return ((int64_t)H * W + kShThreads - 1) / kShThreads; }

size_t shade_sh_workspace_bytes(int B, int H, int W, int n_coeffs)
{
    return (size_t)B * (size_t)shade_sh_chunks(H, W) * (size_t)(3 * n_coeffs) * sizeof(float);
}

// f(std::integral_constant<int, K>) for the K that n_coeffs names (checked by shade_sh_sizes)
template <class F>
void with_sh_coeff_count(int n_coeffs, F f)
{
    if (n_coeffs == 1) f(std::integral_constant<int, 1>());
    else if (n_coeffs == 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 9>());
}

template <int K>
void launch_shade_sh_bwd(const float *colors, const float *normals, int B, int H, int W, const ShadeShArgs &A,
                         const float *grad_pixels, const uint32_t *route, float *grad_colors, float *grad_normals,
                         float *partial, hipStream_t stream)
{
    const dim3 grid((unsigned)shade_sh_chunks(H, W), (unsigned)std::min(B, 65535));  // (at most 8192^2 / 256 chunks)
    if (partial)
        shade_sh_bwd_kernel<K, true><<<grid, dim3(kShThreads), 0, stream>>>(colors, normals, B, H, W, A, grad_pixels,
                                                                            route, grad_colors, grad_normals, partial);
    else
        shade_sh_bwd_kernel<K, false><<<grid, dim3(kShThreads), 0, stream>>>(colors, normals, B, H, W, A, grad_pixels,
                                                                             route, grad_colors, grad_normals, nullptr);
}

}  // namespace

extern "C" {

int dirt_deferred_shade_sh_workspace(int B, int H, int W, int n_coeffs, size_t *bytes)
{
    int64_t n;
    const int rc = shade_sh_sizes(B, H, W, n_coeffs, &n);
    if (rc) return rc;
    if (!bytes) return fail(DIRT_EINVAL, "deferred_shade_sh: null pointer");
    *bytes = shade_sh_workspace_bytes(B, H, W, n_coeffs);
    return DIRT_OK;
}

int dirt_deferred_shade_sh_fwd(const float *colors, const float *normals, const uint8_t *mask, int B, int H, int W,
                               int n_coeffs, int coeffs_per_frame, const float *coefficients, int normalize,
                               float *pixels, uint8_t *valid, uint32_t *route, void *stream_)
{
    int64_t n;
    const int rc = shade_sh_sizes(B, H, W, n_coeffs, &n);
    if (rc || n == 0) return rc;
    if (!colors || !normals || !coefficients || !pixels || !valid || !route)
        return fail(DIRT_EINVAL, "deferred_shade_sh: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeShArgs A = {coefficients, coeffs_per_frame != 0, normalize != 0};
    with_sh_coeff_count(n_coeffs, [&](auto k) {
        shade_sh_fwd_kernel<decltype(k)::value><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
            colors, normals, mask, H, W, n, A, pixels, valid, route);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_shade_sh_bwd(const float *colors, const float *normals, int B, int H, int W, int n_coeffs,
                               int coeffs_per_frame, const float *coefficients, int normalize,
                               const float *grad_pixels, const uint32_t *route, float *grad_colors,
                               float *grad_normals, float *grad_coefficients, void *workspace,
                               size_t workspace_bytes, void *stream_)
{
    int64_t n;
    const int rc = shade_sh_sizes(B, H, W, n_coeffs, &n);
    if (rc || n == 0 || (!grad_colors && !grad_normals && !grad_coefficients)) return rc;
    if (!colors || !normals || !coefficients || !grad_pixels || !route)
        return fail(DIRT_EINVAL, "deferred_shade_sh: null pointer");
    if (grad_coefficients && (!workspace || workspace_bytes < shade_sh_workspace_bytes(B, H, W, n_coeffs)))
        return fail(DIRT_EINVAL, "deferred_shade_sh: workspace smaller than dirt_deferred_shade_sh_workspace() "
                                 "reports");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeShArgs A = {coefficients, coeffs_per_frame != 0, normalize != 0};
    float *partial = grad_coefficients ? static_cast<float *>(workspace) : nullptr;
    with_sh_coeff_count(n_coeffs, [&](auto k) {
        launch_shade_sh_bwd<decltype(k)::value>(colors, normals, B, H, W, A, grad_pixels, route, grad_colors,
                                                grad_normals, partial, stream);
    });
    if (grad_coefficients)
        shade_sh_reduce_kernel<<<dim3((unsigned)(3 * n_coeffs)), dim3(kShThreads), 0, stream>>>(
            partial, B, (int)shade_sh_chunks(H, W), 3 * n_coeffs, coeffs_per_frame != 0, grad_coefficients);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- image-based lighting: the reflection vector and the split-sum combination (shade_env_kernels.h)

namespace {

// the argument checks the entry points share beyond deferred_sizes': DIRT_OK with *pixels = B * H * W
int shade_env_sizes(int B, int H, int W, int n_coeffs, int64_t *pixels)
{
    const int rc = deferred_sizes("deferred_shade_env", B, H, W, 3, pixels);
    if (rc) return rc;
    if (n_coeffs != 1 && n_coeffs != 4 && n_coeffs != 9)
        return fail(DIRT_EINVAL, "deferred_shade_env: expects 1, 4 or 9 coefficients (bands 0, 0-1, 0-2)");
    return DIRT_OK;
}

// both ops' first backward kernel owns kSlThreads pixels a workgroup; a partial row holds `sums` floats
int64_t env_chunks(int H, int W) { return ((int64_t)H * W + kSlThreads - 1) / kSlThreads; }

size_t env_workspace_bytes(int B, int H, int W, int sums)
{
    return (size_t)B * (size_t)env_chunks(H, W) * (size_t)sums * sizeof(float);
}

dim3 env_bwd_grid(int B, int H, int W)
{
    return dim3((unsigned)env_chunks(H, W), (unsigned)std::min(B, 65535));  // (at most 8192^2 / 256 chunks)
}

void launch_env_reduce(const float *partial, int B, int H, int W, int sums, int camera_per_frame, int coeffs_per_frame,
                       const EnvParamGrads &G, hipStream_t stream)
{
    shade_env_reduce_kernel<<<dim3((unsigned)sums), dim3(kSlThreads), 0, stream>>>(
        partial, B, (int)env_chunks(H, W), sums, camera_per_frame != 0, coeffs_per_frame != 0, G);
}

template <int K>
void launch_shade_env_bwd(const float *positions, const float *colors, const float *normals, const float *material,
                          const float *radiance, const float *occlusion, int B, int H, int W, const ShadeEnvArgs &A,
                          const float *grad_pixels, const uint32_t *route, float *grad_positions, float *grad_colors,
                          float *grad_normals, float *grad_material, float *grad_radiance, float *grad_occlusion,
                          float *partial, hipStream_t stream)
{
    const dim3 grid = env_bwd_grid(B, H, W);
    if (partial)
        shade_env_bwd_kernel<K, true><<<grid, dim3(kSlThreads), 0, stream>>>(
            positions, colors, normals, material, radiance, occlusion, B, H, W, A, grad_pixels, route, grad_positions,
            grad_colors, grad_normals, grad_material, grad_radiance, grad_occlusion, partial);
    else
        shade_env_bwd_kernel<K, false><<<grid, dim3(kSlThreads), 0, stream>>>(
            positions, colors, normals, material, radiance, occlusion, B, H, W, A, grad_pixels, route, grad_positions,
            grad_colors, grad_normals, grad_material, grad_radiance, grad_occlusion, nullptr);
}

}  // namespace

extern "C" {

int dirt_deferred_reflect_view_workspace(int B, int H, int W, size_t *bytes)
{
    int64_t n;
    const int rc = deferred_sizes("deferred_reflect_view", B, H, W, 3, &n);
    if (rc) return rc;
    if (!bytes) return fail(DIRT_EINVAL, "deferred_reflect_view: null pointer");
    *bytes = env_workspace_bytes(B, H, W, kEnvCamSums);
    return DIRT_OK;
}

int dirt_deferred_reflect_view_fwd(const float *positions, const float *normals, int B, int H, int W,
                                   int camera_per_frame, const float *camera_position, float *directions,
                                   uint8_t *valid, uint32_t *route, void *stream_)
{
    int64_t n;
    const int rc = deferred_sizes("deferred_reflect_view", B, H, W, 3, &n);
    if (rc || n == 0) return rc;
    if (!positions || !normals || !camera_position || !directions || !valid || !route)
        return fail(DIRT_EINVAL, "deferred_reflect_view: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeEnvArgs A = {camera_position, camera_per_frame != 0, {nullptr, 0, 1}};
    reflect_view_fwd_kernel<<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(positions, normals, H, W, n, A,
                                                                                      directions, valid, route);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_reflect_view_bwd(const float *positions, const float *normals, int B, int H, int W,
                                   int camera_per_frame, const float *camera_position, const float *grad_directions,
                                   const uint32_t *route, float *grad_positions, float *grad_normals,
                                   float *grad_camera, void *workspace, size_t workspace_bytes, void *stream_)
{
    int64_t n;
    const int rc = deferred_sizes("deferred_reflect_view", B, H, W, 3, &n);
    if (rc || n == 0 || (!grad_positions && !grad_normals && !grad_camera)) return rc;
    if (!positions || !normals || !camera_position || !grad_directions || !route)
        return fail(DIRT_EINVAL, "deferred_reflect_view: null pointer");
    if (grad_camera && (!workspace || workspace_bytes < env_workspace_bytes(B, H, W, kEnvCamSums)))
        return fail(DIRT_EINVAL, "deferred_reflect_view: workspace smaller than "
                                 "dirt_deferred_reflect_view_workspace() reports");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeEnvArgs A = {camera_position, camera_per_frame != 0, {nullptr, 0, 1}};
    const dim3 grid = env_bwd_grid(B, H, W);
    if (grad_camera) {
        float *partial = static_cast<float *>(workspace);
        reflect_view_bwd_kernel<true><<<grid, dim3(kSlThreads), 0, stream>>>(
            positions, normals, B, H, W, A, grad_directions, route, grad_positions, grad_normals, partial);
        launch_env_reduce(partial, B, H, W, kEnvCamSums, camera_per_frame, 0, {grad_camera, nullptr}, stream);
    } else {
        reflect_view_bwd_kernel<false><<<grid, dim3(kSlThreads), 0, stream>>>(
            positions, normals, B, H, W, A, grad_directions, route, grad_positions, grad_normals, nullptr);
    }
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_shade_env_workspace(int B, int H, int W, int n_coeffs, size_t *bytes)
{
    int64_t n;
    const int rc = shade_env_sizes(B, H, W, n_coeffs, &n);
    if (rc) return rc;
    if (!bytes) return fail(DIRT_EINVAL, "deferred_shade_env: null pointer");
    *bytes = env_workspace_bytes(B, H, W, kEnvCamSums + 3 * n_coeffs);
    return DIRT_OK;
}

int dirt_deferred_shade_env_fwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *radiance, const float *occlusion, int B, int H,
                                int W, int n_coeffs, int coeffs_per_frame, const float *coefficients,
                                int camera_per_frame, const float *camera_position, float *pixels, uint8_t *valid,
                                uint32_t *route, void *stream_)
{
    int64_t n;
    const int rc = shade_env_sizes(B, H, W, n_coeffs, &n);
    if (rc || n == 0) return rc;
    if (!positions || !colors || !normals || !material || !radiance || !coefficients || !camera_position || !pixels ||
        !valid || !route)
        return fail(DIRT_EINVAL, "deferred_shade_env: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeEnvArgs A = {camera_position, camera_per_frame != 0, {coefficients, coeffs_per_frame != 0, 1}};
    with_sh_coeff_count(n_coeffs, [&](auto k) {
        shade_env_fwd_kernel<decltype(k)::value><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
            positions, colors, normals, material, radiance, occlusion, H, W, n, A, pixels, valid, route);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_deferred_shade_env_bwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *radiance, const float *occlusion, int B, int H,
                                int W, int n_coeffs, int coeffs_per_frame, const float *coefficients,
                                int camera_per_frame, const float *camera_position, const float *grad_pixels,
                                const uint32_t *route, float *grad_positions, float *grad_colors, float *grad_normals,
                                float *grad_material, float *grad_radiance, float *grad_occlusion,
                                float *grad_coefficients, float *grad_camera, void *workspace, size_t workspace_bytes,
                                void *stream_)
{
    int64_t n;
    const int rc = shade_env_sizes(B, H, W, n_coeffs, &n);
    if (rc || n == 0) return rc;
    if (!occlusion) grad_occlusion = nullptr;  // (ones: nothing to receive it)
    const bool want_params = grad_coefficients || grad_camera;
    if (!want_params && !grad_positions && !grad_colors && !grad_normals && !grad_material && !grad_radiance &&
        !grad_occlusion)
        return DIRT_OK;
    if (!positions || !colors || !normals || !material || !radiance || !coefficients || !camera_position ||
        !grad_pixels || !route)
        return fail(DIRT_EINVAL, "deferred_shade_env: null pointer");
    const int sums = kEnvCamSums + 3 * n_coeffs;
    if (want_params && (!workspace || workspace_bytes < env_workspace_bytes(B, H, W, sums)))
        return fail(DIRT_EINVAL, "deferred_shade_env: workspace smaller than "
                                 "dirt_deferred_shade_env_workspace() reports");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const ShadeEnvArgs A = {camera_position, camera_per_frame != 0, {coefficients, coeffs_per_frame != 0, 1}};
    float *partial = want_params ? static_cast<float *>(workspace) : nullptr;
    with_sh_coeff_count(n_coeffs, [&](auto k) {
        launch_shade_env_bwd<decltype(k)::value>(positions, colors, normals, material, radiance, occlusion, B, H, W, A,
                                                 grad_pixels, route, grad_positions, grad_colors, grad_normals,
                                                 grad_material, grad_radiance, grad_occlusion, partial, stream);
    });
    if (want_params)
        launch_env_reduce(partial, B, H, W, sums, camera_per_frame, coeffs_per_frame,
                          {grad_camera, grad_coefficients}, stream);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- deferred texturing: bilinear texture sampling and its gradients (texture_kernels.h)

namespace {

struct SampleGrid {
    int64_t pixels;        // B * H * W (0: nothing to do)
    int tiles_x, tiles_y;  // the backward's kTexTile x kTexTile screen tiles over one frame
};

int texture_dims(const char *op, int Th, int Tw)
{
    if (Th < 1 || Tw < 1 || Th > DIRT_MAX_DIM || Tw > DIRT_MAX_DIM) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: texture height, width must be in 1..%d", op, DIRT_MAX_DIM);
        return fail(DIRT_EINVAL, msg);
    }
    return DIRT_OK;
}

// the argument checks that the plain and the mip sample entry points share beyond deferred_sizes' and the texture's
// own: the wrap, the texture's frames against the batch, the tiles of one launch; DIRT_OK with g's tile grid
int sample_sizes(const char *op, int texture_frames, int B, int H, int W, int wrap, SampleGrid *g)
{
    const auto bad = [op](const char *what) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: %s", op, what);
        return fail(DIRT_EINVAL, msg);
    };
    if (wrap != DIRT_TEXTURE_CLAMP && wrap != DIRT_TEXTURE_REPEAT)
        return bad("wrap must be DIRT_TEXTURE_CLAMP or DIRT_TEXTURE_REPEAT");
    if (B > 0 && texture_frames != 1 && texture_frames != B) return bad("texture_frames must be 1 or the batch size");
    g->tiles_x = (W + kTexTile - 1) / kTexTile;
    g->tiles_y = (H + kTexTile - 1) / kTexTile;
    if ((int64_t)B * g->tiles_y * g->tiles_x > 0x7fffffffLL)
        return bad("too large (more screen tiles than one launch covers)");
    return DIRT_OK;
}

int texture_sizes(int texture_frames, int Th, int Tw, int B, int H, int W, int C, int wrap, SampleGrid *g)
{
    int rc = deferred_sizes("texture_sample", B, H, W, C, &g->pixels);
    if (!rc) rc = texture_dims("texture_sample", Th, Tw);
    if (!rc) rc = sample_sizes("texture_sample", texture_frames, B, H, W, wrap, g);
    if (rc) g->pixels = 0;
    return rc;
}

template <int C>
void launch_texture_fwd(const float *texture, int64_t frame_stride, int Th, int Tw, const float *uv,
                        const uint8_t *mask, int64_t hw, int64_t n, int wrap, float *texels, uint8_t *valid,
                        hipStream_t stream)
{
    texture_sample_fwd_kernel<C><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        texture, frame_stride, Th, Tw, uv, mask, hw, n, wrap, texels, valid);
}

template <int C>
void launch_texture_bwd(const float *texture, int64_t frame_stride, int Th, int Tw, const float *uv,
                        const uint8_t *mask, int B, int H, int W, SampleGrid g, int wrap, const float *grad,
                        float *grad_texture, float *grad_uv, hipStream_t stream)
{
    texture_sample_bwd_kernel<C>
        <<<dim3((unsigned)((int64_t)B * g.tiles_y * g.tiles_x)), dim3(kLightThreads), 0, stream>>>(
            texture, frame_stride, Th, Tw, uv, mask, H, W, g.tiles_x, g.tiles_y, wrap, grad, grad_texture, grad_uv);
}

}  // namespace

extern "C" {

int dirt_texture_sample_fwd(const float *texture, int texture_frames, int Th, int Tw, int C, const float *uv,
                            const uint8_t *mask, int B, int H, int W, int wrap, float *texels, uint8_t *valid,
                            void *stream_)
{
    SampleGrid g;
    const int rc = texture_sizes(texture_frames, Th, Tw, B, H, W, C, wrap, &g);
    if (rc || g.pixels == 0) return rc;
    if (!texture || !uv || !texels || !valid) return fail(DIRT_EINVAL, "texture_sample: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = texture_frames == 1 ? 0 : (int64_t)Th * Tw * C, hw = (int64_t)H * W;
    with_each_channel_count(C, [&](auto c) {
        launch_texture_fwd<decltype(c)::value>(texture, fs, Th, Tw, uv, mask, hw, g.pixels, wrap, texels, valid, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_texture_sample_bwd(const float *texture, int texture_frames, int Th, int Tw, int C, const float *uv,
                            const uint8_t *mask, int B, int H, int W, int wrap, const float *grad_texels,
                            float *grad_texture, float *grad_uv, void *stream_)
{
    SampleGrid g;
    const int rc = texture_sizes(texture_frames, Th, Tw, B, H, W, C, wrap, &g);
    if (rc || g.pixels == 0 || (!grad_texture && !grad_uv)) return rc;
    if (!texture || !uv || !grad_texels) return fail(DIRT_EINVAL, "texture_sample: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = texture_frames == 1 ? 0 : (int64_t)Th * Tw * C;
    if (grad_texture)
        HIP_TRY(hipMemsetAsync(grad_texture, 0, (size_t)texture_frames * Th * Tw * C * sizeof(float), stream));
    with_each_channel_count(C, [&](auto c) {
        launch_texture_bwd<decltype(c)::value>(texture, fs, Th, Tw, uv, mask, B, H, W, g, wrap, grad_texels,
                                               grad_texture, grad_uv, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- mipmapped deferred texturing: the chain build, the trilinear lookup and their gradients (texture_mip_kernels.h)

namespace {

// number of levels of the chain of a Th x Tw texture, truncated to max_levels when that is positive
int mip_chain_length(int Th, int Tw, int max_levels)
{
    int L = 1, h = Th, w = Tw;
    while (L < kMaxMipLevels && (max_levels <= 0 || L < max_levels) && !(h == 1 && w == 1) &&
           (h == 1 || h % 2 == 0) && (w == 1 || w % 2 == 0)) {
        h = h > 1 ? h / 2 : 1;
        w = w > 1 ? w / 2 : 1;
        ++L;
    }
    return L;
}

// the texture-side argument checks of the mip entry points: DIRT_OK with *L the number of levels (levels <= 0: the
// whole chain) and *texels the texels of one frame of the packed chain
int mip_sizes(const char *op, int texture_frames, int Th, int Tw, int C, int levels, int *L, int64_t *texels)
{
    char msg[160];
    const int rc = texture_dims(op, Th, Tw);
    if (rc) return rc;
    if (C < 1 || C > DIRT_MAX_CHANNELS) {
        snprintf(msg, sizeof(msg), "%s: expects 1 <= channels <= %d", op, DIRT_MAX_CHANNELS);
        return fail(DIRT_EINVAL, msg);
    }
    if (texture_frames < 0) {
        snprintf(msg, sizeof(msg), "%s: texture_frames must be non-negative", op);
        return fail(DIRT_EINVAL, msg);
    }
    const int full = mip_chain_length(Th, Tw, 0);
    if (levels > full) {
        snprintf(msg, sizeof(msg), "%s: levels = %d, but the chain of a %d x %d texture has %d", op, levels, Th, Tw,
                 full);
        return fail(DIRT_EINVAL, msg);
    }
    *L = levels <= 0 ? full : levels;
    *texels = mip_level(Th, Tw, *L).off;
    if (((int64_t)texture_frames * Th * Tw * C + kLightThreads - 1) / kLightThreads > 0x7fffffffLL) {
        snprintf(msg, sizeof(msg), "%s: too large (more texture elements than one launch covers)", op);
        return fail(DIRT_EINVAL, msg);
    }
    return DIRT_OK;
}

int mip_sample_sizes(int texture_frames, int Th, int Tw, int C, int levels, int B, int H, int W, int wrap, int *L,
                     int64_t *texels, SampleGrid *g)
{
    int rc = deferred_sizes("texture_sample_mip", B, H, W, C, &g->pixels);
    if (!rc) rc = mip_sizes("texture_sample_mip", texture_frames, Th, Tw, C, levels, L, texels);
    if (!rc) rc = sample_sizes("texture_sample_mip", texture_frames, B, H, W, wrap, g);
    if (rc) g->pixels = 0;
    return rc;
}

template <int C>
void launch_texture_mip_fwd(const float *packed, int64_t frame_stride, int Th, int Tw, int L, const float *uv,
                            const uint8_t *mask, const float *lod_in, float lod_bias, int H, int W, int64_t n, int wrap,
                            float *texels, uint8_t *valid, float *lod, hipStream_t stream)
{
    texture_sample_mip_fwd_kernel<C><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        packed, frame_stride, Th, Tw, L, uv, mask, lod_in, lod_bias, H, W, n, wrap, texels, valid, lod);
}

template <int C>
void launch_texture_mip_bwd(const float *packed, int64_t frame_stride, int Th, int Tw, int L, const float *uv,
                            const uint8_t *mask, const float *lod, int B, int H, int W, SampleGrid g, int wrap,
                            const float *grad, float *grad_packed, float *grad_uv, hipStream_t stream)
{
    texture_sample_mip_bwd_kernel<C>
        <<<dim3((unsigned)((int64_t)B * g.tiles_y * g.tiles_x)), dim3(kLightThreads), 0, stream>>>(
            packed, frame_stride, Th, Tw, L, uv, mask, lod, H, W, g.tiles_x, g.tiles_y, wrap, grad, grad_packed,
            grad_uv);
}

}  // namespace

extern "C" {

int dirt_texture_mip_layout(int Th, int Tw, int max_levels, int *dims, long long *offsets, long long *total)
{
    if (texture_dims("texture_mip_layout", Th, Tw)) return 0;
    const int L = mip_chain_length(Th, Tw, max_levels);
    MipLevel lv = mip_level(Th, Tw, 0);
    for (int k = 0; k < L; ++k, lv = mip_next(lv)) {
        if (dims) {
            dims[2 * k] = lv.h;
            dims[2 * k + 1] = lv.w;
        }
        if (offsets) offsets[k] = lv.off;
    }
    if (total) *total = lv.off;
    return L;
}

int dirt_texture_mip_build_fwd(const float *texture, int texture_frames, int Th, int Tw, int C, int levels,
                               float *packed, void *stream_)
{
    int L;
    int64_t N;
    const int rc = mip_sizes("texture_mip_build", texture_frames, Th, Tw, C, levels, &L, &N);
    if (rc || texture_frames == 0) return rc;
    if (!texture || !packed) return fail(DIRT_EINVAL, "texture_mip_build: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = N * C, n0 = (int64_t)Th * Tw * C;
    mip_copy_kernel<<<dim3(light_blocks(texture_frames * n0)), dim3(kLightThreads), 0, stream>>>(
        texture, n0, fs, texture_frames * n0, packed);
    MipLevel src = mip_level(Th, Tw, 0);
    for (int k = 1; k < L; ++k) {
        const MipLevel dst = mip_next(src);
        const int64_t n = (int64_t)texture_frames * dst.h * dst.w * C;
        mip_down_kernel<<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
            packed, fs, src.off * C, src.h, src.w, dst.off * C, dst.h, dst.w, C, n);
        src = dst;
    }
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_texture_mip_build_bwd(const float *grad_packed, int texture_frames, int Th, int Tw, int C, int levels,
                               float *grad_texture, void *stream_)
{
    int L;
    int64_t N;
    const int rc = mip_sizes("texture_mip_build", texture_frames, Th, Tw, C, levels, &L, &N);
    if (rc || texture_frames == 0) return rc;
    if (!grad_packed || !grad_texture) return fail(DIRT_EINVAL, "texture_mip_build: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t n = (int64_t)texture_frames * Th * Tw * C;
    mip_build_bwd_kernel<<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(grad_packed, N * C, Th, Tw, C, L, n,
                                                                                    grad_texture);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_texture_sample_mip_fwd(const float *packed, int texture_frames, int Th, int Tw, int C, int levels,
                                const float *uv, const uint8_t *mask, const float *lod_in, float lod_bias, int B, int H,
                                int W, int wrap, float *texels, uint8_t *valid, float *lod, void *stream_)
{
    int L;
    int64_t N;
    SampleGrid g;
    const int rc = mip_sample_sizes(texture_frames, Th, Tw, C, levels, B, H, W, wrap, &L, &N, &g);
    if (rc || g.pixels == 0) return rc;
    if (!(lod_bias - lod_bias == 0.0f)) return fail(DIRT_EINVAL, "texture_sample_mip: lod_bias must be finite");
    if (!packed || !uv || !texels || !valid || !lod) return fail(DIRT_EINVAL, "texture_sample_mip: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = texture_frames == 1 ? 0 : N * C;
    with_each_channel_count(C, [&](auto c) {
        launch_texture_mip_fwd<decltype(c)::value>(packed, fs, Th, Tw, L, uv, mask, lod_in, lod_bias, H, W, g.pixels,
                                                   wrap, texels, valid, lod, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_texture_sample_mip_bwd(const float *packed, int texture_frames, int Th, int Tw, int C, int levels,
                                const float *uv, const uint8_t *mask, const float *lod, int B, int H, int W, int wrap,
                                const float *grad_texels, float *grad_packed, float *grad_uv, void *stream_)
{
    int L;
    int64_t N;
    SampleGrid g;
    const int rc = mip_sample_sizes(texture_frames, Th, Tw, C, levels, B, H, W, wrap, &L, &N, &g);
    if (rc || g.pixels == 0 || (!grad_packed && !grad_uv)) return rc;
    if (!packed || !uv || !lod || !grad_texels) return fail(DIRT_EINVAL, "texture_sample_mip: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = texture_frames == 1 ? 0 : N * C;
    if (grad_packed) HIP_TRY(hipMemsetAsync(grad_packed, 0, (size_t)texture_frames * N * C * sizeof(float), stream));
    with_each_channel_count(C, [&](auto c) {
        launch_texture_mip_bwd<decltype(c)::value>(packed, fs, Th, Tw, L, uv, mask, lod, B, H, W, g, wrap, grad_texels,
                                                   grad_packed, grad_uv, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- cube-map lookup at a direction G-buffer and its gradients (cubemap_kernels.h)

namespace {

int cube_sizes(int cubemap_frames, int S, int C, int B, int H, int W, SampleGrid *g)
{
    const char *op = "texture_sample_cube";
    char msg[160];
    int rc = deferred_sizes(op, B, H, W, C, &g->pixels);
    if (!rc && (S < 1 || S > DIRT_MAX_DIM)) {
        snprintf(msg, sizeof(msg), "%s: the faces' size must be in 1..%d", op, DIRT_MAX_DIM);
        rc = fail(DIRT_EINVAL, msg);
    }
    if (!rc && B > 0 && cubemap_frames != 1 && cubemap_frames != B) {
        snprintf(msg, sizeof(msg), "%s: cubemap_frames must be 1 or the batch size", op);
        rc = fail(DIRT_EINVAL, msg);
    }
    if (!rc) rc = sample_sizes(op, 1, B, H, W, DIRT_TEXTURE_CLAMP, g);
    if (rc) g->pixels = 0;
    return rc;
}

template <int C>
void launch_cubemap_fwd(const float *cubemap, int64_t frame_stride, int S, const float *directions,
                        const uint8_t *mask, int64_t hw, int64_t n, float *texels, uint8_t *valid, hipStream_t stream)
{
    cubemap_sample_fwd_kernel<C><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        cubemap, frame_stride, S, directions, mask, hw, n, texels, valid);
}

template <int C>
void launch_cubemap_bwd(const float *cubemap, int64_t frame_stride, int S, const float *directions,
                        const uint8_t *mask, int B, int H, int W, SampleGrid g, const float *grad, float *grad_cubemap,
                        float *grad_directions, hipStream_t stream)
{
    cubemap_sample_bwd_kernel<C>
        <<<dim3((unsigned)((int64_t)B * g.tiles_y * g.tiles_x)), dim3(kLightThreads), 0, stream>>>(
            cubemap, frame_stride, S, directions, mask, H, W, g.tiles_x, g.tiles_y, grad, grad_cubemap, grad_directions);
}

}  // namespace

extern "C" {

int dirt_texture_sample_cube_fwd(const float *cubemap, int cubemap_frames, int S, int C, const float *directions,
                                 const uint8_t *mask, int B, int H, int W, float *texels, uint8_t *valid, void *stream_)
{
    SampleGrid g;
    const int rc = cube_sizes(cubemap_frames, S, C, B, H, W, &g);
    if (rc || g.pixels == 0) return rc;
    if (!cubemap || !directions || !texels || !valid) return fail(DIRT_EINVAL, "texture_sample_cube: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = cubemap_frames == 1 ? 0 : (int64_t)6 * S * S * C, hw = (int64_t)H * W;
    with_each_channel_count(C, [&](auto c) {
        launch_cubemap_fwd<decltype(c)::value>(cubemap, fs, S, directions, mask, hw, g.pixels, texels, valid, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_texture_sample_cube_bwd(const float *cubemap, int cubemap_frames, int S, int C, const float *directions,
                                 const uint8_t *mask, int B, int H, int W, const float *grad_texels,
                                 float *grad_cubemap, float *grad_directions, void *stream_)
{
    SampleGrid g;
    const int rc = cube_sizes(cubemap_frames, S, C, B, H, W, &g);
    if (rc || g.pixels == 0 || (!grad_cubemap && !grad_directions)) return rc;
    if (!cubemap || !directions || !grad_texels) return fail(DIRT_EINVAL, "texture_sample_cube: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = cubemap_frames == 1 ? 0 : (int64_t)6 * S * S * C;
    if (grad_cubemap)
        HIP_TRY(hipMemsetAsync(grad_cubemap, 0, (size_t)cubemap_frames * 6 * S * S * C * sizeof(float), stream));
    with_each_channel_count(C, [&](auto c) {
        launch_cubemap_bwd<decltype(c)::value>(cubemap, fs, S, directions, mask, B, H, W, g, grad_texels, grad_cubemap,
                                               grad_directions, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- seamless mip-mapped cube-map lookup and its gradients (cubemap_mip_kernels.h)

namespace {

// the argument checks of the two entry points: DIRT_OK with *L the number of levels (levels <= 0: the whole chain) and
// *texels the texels of one face's chain
int cube_mip_sizes(int cubemap_frames, int S, int C, int levels, int B, int H, int W, int seamless, int *L,
                   int64_t *texels, SampleGrid *g)
{
    const char *op = "texture_sample_cube_mip";
    int rc = cube_sizes(cubemap_frames, S, C, B, H, W, g);
    if (!rc) rc = mip_sizes(op, 6 * (cubemap_frames > 0 ? cubemap_frames : 0), S, S, C, levels, L, texels);
    if (!rc && seamless != 0 && seamless != 1)
        rc = fail(DIRT_EINVAL, "texture_sample_cube_mip: seamless must be 0 or 1");
    if (rc) g->pixels = 0;
    return rc;
}

template <int C>
void launch_cubemap_mip_fwd(const float *packed, int64_t frame_stride, int64_t n_face, int S, int L,
                            const float *directions, const uint8_t *mask, const float *lod_in, float lod_bias, int H,
                            int W, int64_t n, int seamless, float *texels, uint8_t *valid, float *lod,
                            hipStream_t stream)
{
    cubemap_sample_mip_fwd_kernel<C><<<dim3(light_blocks(n)), dim3(kLightThreads), 0, stream>>>(
        packed, frame_stride, n_face, S, L, directions, mask, lod_in, lod_bias, H, W, n, seamless, texels, valid, lod);
}

template <int C>
void launch_cubemap_mip_bwd(const float *packed, int64_t frame_stride, int64_t n_face, int S, int L,
                            const float *directions, const uint8_t *mask, const float *lod_in, float lod_bias,
                            const float *lod, int B, int H, int W, SampleGrid g, int seamless, const float *grad,
                            float *grad_packed, float *grad_directions, float *grad_lod, hipStream_t stream)
{
    cubemap_sample_mip_bwd_kernel<C>
        <<<dim3((unsigned)((int64_t)B * g.tiles_y * g.tiles_x)), dim3(kLightThreads), 0, stream>>>(
            packed, frame_stride, n_face, S, L, directions, mask, lod_in, lod_bias, lod, H, W, g.tiles_x, g.tiles_y,
            seamless, grad, grad_packed, grad_directions, grad_lod);
}

}  // namespace

extern "C" {

int dirt_texture_sample_cube_mip_fwd(const float *packed, int cubemap_frames, int S, int C, int levels,
                                     const float *directions, const uint8_t *mask, const float *lod_in, float lod_bias,
                                     int B, int H, int W, int seamless, float *texels, uint8_t *valid, float *lod,
                                     void *stream_)
{
    int L;
    int64_t N;
    SampleGrid g;
    const int rc = cube_mip_sizes(cubemap_frames, S, C, levels, B, H, W, seamless, &L, &N, &g);
    if (rc) return rc;
    if (!(lod_bias - lod_bias == 0.0f)) return fail(DIRT_EINVAL, "texture_sample_cube_mip: lod_bias must be finite");
    if (g.pixels == 0) return DIRT_OK;
    if (!packed || !directions || !texels || !valid || !lod)
        return fail(DIRT_EINVAL, "texture_sample_cube_mip: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = cubemap_frames == 1 ? 0 : 6 * N * C;
    with_each_channel_count(C, [&](auto c) {
        launch_cubemap_mip_fwd<decltype(c)::value>(packed, fs, N, S, L, directions, mask, lod_in, lod_bias, H, W,
                                                   g.pixels, seamless, texels, valid, lod, stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_texture_sample_cube_mip_bwd(const float *packed, int cubemap_frames, int S, int C, int levels,
                                     const float *directions, const uint8_t *mask, const float *lod_in, float lod_bias,
                                     const float *lod, int B, int H, int W, int seamless, const float *grad_texels,
                                     float *grad_packed, float *grad_directions, float *grad_lod, void *stream_)
{
    int L;
    int64_t N;
    SampleGrid g;
    const int rc = cube_mip_sizes(cubemap_frames, S, C, levels, B, H, W, seamless, &L, &N, &g);
    if (rc) return rc;
    if (!(lod_bias - lod_bias == 0.0f)) return fail(DIRT_EINVAL, "texture_sample_cube_mip: lod_bias must be finite");
    if (grad_lod && !lod_in)
        return fail(DIRT_EINVAL, "texture_sample_cube_mip: grad_lod needs the explicit lod_in it is the gradient of");
    if (g.pixels == 0 || (!grad_packed && !grad_directions && !grad_lod)) return DIRT_OK;
    if (!packed || !directions || !lod || !grad_texels)
        return fail(DIRT_EINVAL, "texture_sample_cube_mip: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = cubemap_frames == 1 ? 0 : 6 * N * C;
    if (grad_packed)
        HIP_TRY(hipMemsetAsync(grad_packed, 0, (size_t)cubemap_frames * 6 * N * C * sizeof(float), stream));
    with_each_channel_count(C, [&](auto c) {
        launch_cubemap_mip_bwd<decltype(c)::value>(packed, fs, N, S, L, directions, mask, lod_in, lod_bias, lod, B, H,
                                                   W, g, seamless, grad_texels, grad_packed, grad_directions, grad_lod,
                                                   stream);
    });
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"

// ---- shadow-map lookup at a position G-buffer and its gradients (shadow_kernels.h)

namespace {

// the argument checks of the three entry points: DIRT_OK with g's pixel count and tile grid
int shadow_sizes(int map_frames, int Sh, int Sw, int B, int H, int W, float bias, float softness, SampleGrid *g)
{
    const char *op = "shadow_sample";
    int rc = deferred_sizes(op, B, H, W, 1, &g->pixels);
    if (!rc && (Sh < 1 || Sw < 1 || Sh > DIRT_MAX_DIM || Sw > DIRT_MAX_DIM)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: depth map height, width must be in 1..%d", op, DIRT_MAX_DIM);
        rc = fail(DIRT_EINVAL, msg);
    }
    if (!rc && !(bias >= 0.0f && bias - bias == 0.0f && softness >= 0.0f && softness - softness == 0.0f))
        rc = fail(DIRT_EINVAL, "shadow_sample: bias and softness must be finite and non-negative");
    if (!rc && B > 0 && map_frames != 1 && map_frames != B)
        rc = fail(DIRT_EINVAL, "shadow_sample: map_frames must be 1 or the batch size");
    if (!rc) rc = sample_sizes(op, map_frames, B, H, W, DIRT_TEXTURE_CLAMP, g);
    if (rc) g->pixels = 0;
    return rc;
}

size_t shadow_workspace_bytes(int B, const SampleGrid &g)
{
    return (size_t)B * (size_t)g.tiles_y * (size_t)g.tiles_x * kShadowSums * sizeof(float);
}

ShadowArgs shadow_args(const float *light_matrix, int matrix_per_frame, float bias, float softness)
{
    return {light_matrix, matrix_per_frame != 0, bias, softness, softness > 0.0f ? 1.0f / softness : 0.0f};
}

}  // namespace

extern "C" {

int dirt_shadow_sample_workspace(int B, int H, int W, size_t *bytes)
{
    SampleGrid g;
    const int rc = shadow_sizes(1, 1, 1, B, H, W, 0.0f, 0.0f, &g);
    if (rc) return rc;
    if (!bytes) return fail(DIRT_EINVAL, "shadow_sample: null pointer");
    *bytes = shadow_workspace_bytes(B, g);
    return DIRT_OK;
}

int dirt_shadow_sample_fwd(const float *depth_map, int map_frames, int Sh, int Sw, const float *positions,
                           const uint8_t *mask, int B, int H, int W, int matrix_per_frame, const float *light_matrix,
                           float bias, float softness, float *visibility, uint8_t *valid, void *stream_)
{
    SampleGrid g;
    const int rc = shadow_sizes(map_frames, Sh, Sw, B, H, W, bias, softness, &g);
    if (rc || g.pixels == 0) return rc;
    if (!depth_map || !positions || !light_matrix || !visibility || !valid)
        return fail(DIRT_EINVAL, "shadow_sample: null pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = map_frames == 1 ? 0 : (int64_t)Sh * Sw;
    shadow_sample_fwd_kernel<<<dim3(light_blocks(g.pixels)), dim3(kLightThreads), 0, stream>>>(
        depth_map, fs, Sh, Sw, positions, mask, (int64_t)H * W, g.pixels,
        shadow_args(light_matrix, matrix_per_frame, bias, softness), visibility, valid);
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

int dirt_shadow_sample_bwd(const float *depth_map, int map_frames, int Sh, int Sw, const float *positions,
                           const uint8_t *mask, int B, int H, int W, int matrix_per_frame, const float *light_matrix,
                           float bias, float softness, const float *grad_visibility, float *grad_depth_map,
                           float *grad_positions, float *grad_light_matrix, void *workspace, size_t workspace_bytes,
                           void *stream_)
{
    SampleGrid g;
    const int rc = shadow_sizes(map_frames, Sh, Sw, B, H, W, bias, softness, &g);
    if (rc || g.pixels == 0 || (!grad_depth_map && !grad_positions && !grad_light_matrix)) return rc;
    if (!depth_map || !positions || !light_matrix || !grad_visibility)
        return fail(DIRT_EINVAL, "shadow_sample: null pointer");
    if (grad_light_matrix && (!workspace || workspace_bytes < shadow_workspace_bytes(B, g)))
        return fail(DIRT_EINVAL, "shadow_sample: workspace smaller than dirt_shadow_sample_workspace() reports");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t fs = map_frames == 1 ? 0 : (int64_t)Sh * Sw;
    if (grad_depth_map)
        HIP_TRY(hipMemsetAsync(grad_depth_map, 0, (size_t)map_frames * Sh * Sw * sizeof(float), stream));
    const ShadowArgs A = shadow_args(light_matrix, matrix_per_frame, bias, softness);
    const int64_t tiles = (int64_t)g.tiles_y * g.tiles_x;
    const dim3 grid((unsigned)((int64_t)B * tiles));
    float *partial = static_cast<float *>(workspace);
    if (grad_light_matrix) {
        shadow_sample_bwd_kernel<true><<<grid, dim3(kLightThreads), 0, stream>>>(
            depth_map, fs, Sh, Sw, positions, mask, H, W, g.tiles_x, g.tiles_y, A, grad_visibility, grad_depth_map,
            grad_positions, partial);
        shadow_reduce_kernel<<<dim3(kShadowSums), dim3(kSlThreads), 0, stream>>>(partial, B, tiles,
                                                                                 matrix_per_frame != 0,
                                                                                 grad_light_matrix);
    } else {
        shadow_sample_bwd_kernel<false><<<grid, dim3(kLightThreads), 0, stream>>>(
            depth_map, fs, Sh, Sw, positions, mask, H, W, g.tiles_x, g.tiles_y, A, grad_visibility, grad_depth_map,
            grad_positions, nullptr);
    }
    HIP_TRY(hipGetLastError());
    return DIRT_OK;
}

}  // extern "C"
