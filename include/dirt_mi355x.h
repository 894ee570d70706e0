/*
 * dirt_mi355x.h -- C ABI of the MI355X-native dirt rasteriser (libdirt_mi355x.so).
 *
 * Drop-in boundary for the reference's TensorFlow custom ops in librasterise.so
 * (loaded by tf.load_op_library at dirt/rasterise_ops.py:7):
 *
 *   dirt_rasterise_fwd  replaces  REGISTER_OP("Rasterise")           csrc/rasterise_egl.cpp:33-53
 *                                 RasteriseOpGpu::Compute            csrc/rasterise_egl.cpp:284-514
 *                                 upload_background/download_pixels  csrc/rasterise_egl.cu:16-129
 *   dirt_rasterise_bwd  replaces  launch_grad_assembly (declared,    csrc/rasterise_grad_common.h:19-24
 *                                 never defined in the fork) -- the gradient DIRT registers upstream
 *                                 for "Rasterise"; the fork's REGISTER_OP("RasteriseGrad")
 *                                 (csrc/rasterise_grad_egl.cpp:33-53) is a forward render
 *   dirt_rasterise_bwd_recompute  the same gradient from the op's inputs + output + grad_pixels only, for
 *                                 a single-output `Rasterise` with tf.RegisterGradient (upstream DIRT's
 *                                 shape: rasterise_grad_common.h:5-24 re-derives its G-buffer)
 *   dirt_hill_fwd       replaces  REGISTER_OP("Hill") + HillOpGpu     csrc/hill.cpp:33-53, 282-498
 *                                 (the other procedural ops are shader ids of dirt_rasterise_fwd:
 *                                 RasteriseGrad, OceanicStillCloud, OceanicNoCloud, OceanicOptFlow,
 *                                 OceanicSimpleProxy -- csrc/rasterise_grad_egl.cpp, csrc/oceanic_*.cpp)
 *   dirt_last_error     replaces  OP_REQUIRES(..., errors::InvalidArgument(...)) messages,
 *                                 csrc/rasterise_egl.cpp:310-336 (the reference aborts on everything
 *                                 else via LOG(FATAL)/CHECK; this ABI never aborts)
 *
 * Conventions
 *   - every tensor pointer is a DEVICE pointer to a dense row-major array (HBM of the current HIP device);
 *   - float32 data, int32 faces; shapes use the reference's batch-leading layout
 *       background    [B,H,W,C]   top row first (rasterise_egl.cu:29)
 *       vertices      [B,V,4]     OpenGL clip space x,y,z,w (README.md:131)
 *       vertex_colors [B,V,C]
 *       faces         [B,F,3]     indices into the same frame's vertices (base vertex b*V, rasterise_egl.cpp:457)
 *       pixels        [B,H,W,C]   output
 *   - outputs are caller-owned; work is enqueued asynchronously on `stream` (a hipStream_t, 0 = null stream);
 *   - `saved` is the state the backward needs (per-face setup records); `scratch` is forward-only
 *     (tile bins).  Query their sizes with dirt_workspace_sizes; the caller owns both.
 *   - channels C may be 1..DIRT_MAX_CHANNELS (the reference accepts 1 or 3, csrc/hwc.h:27).
 *
 * Return codes: DIRT_OK, DIRT_EINVAL (bad shape/argument; message in dirt_last_error()),
 * DIRT_EHIP (a HIP runtime error).  Out-of-range face indices cull the face (the reference reads
 * out of bounds); dirt_check_faces() reports them on request.
 */
#ifndef DIRT_MI355X_H
#define DIRT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIRT_OK 0
#define DIRT_EINVAL 1
#define DIRT_EFACE 2
#define DIRT_EHIP 3

#define DIRT_MAX_CHANNELS 8
#define DIRT_MAX_DIM 8192

/* fragment programs (shader_id); 0 = Gouraud (README.md:134-137) */
#define DIRT_SHADER_GOURAUD 0
#define DIRT_SHADER_OCEANIC_HORIZON 1 /* csrc/shaders.cpp:1668-1919 (the fork's `Rasterise` program) */
#define DIRT_SHADER_OCEANIC 2             /* csrc/shaders.cpp:556-864 (`RasteriseGrad`, rasterise_grad_egl.cpp:399) */
#define DIRT_SHADER_OCEANIC_STILL_CLOUD 3 /* csrc/shaders.cpp:866-1176 (`OceanicStillCloud`; camera_pos[8] = cloud_t) */
#define DIRT_SHADER_OCEANIC_NO_CLOUD 4    /* csrc/shaders.cpp:1402-1666 (`OceanicNoCloud`) */
#define DIRT_SHADER_OCEANIC_SIMPLE_PROXY 5 /* csrc/shaders.cpp:1921-2185 (`OceanicSimpleProxy`) */
#define DIRT_SHADER_OCEANIC_OPT_FLOW 6 /* csrc/shaders.cpp:1178-1398 (`OceanicOptFlow`; camera_pos: 16 floats,
                                          oceanic_opt_flow.cpp:399-414); pixels = previous-frame coordinates */
#define DIRT_SHADER_HILL 7 /* csrc/shaders.cpp:123-554 (`Hill`, csrc/hill.cpp; camera_pos: 12 floats); no depth
                              test (last face wins), background = terrain lookup, uncovered pixels 0 */

/* ABI version, bumped on any signature or workspace-layout change (4: + dirt_hill_fwd, shader ids 6 and 7;
 * 5: setup bins directly into fixed-capacity per-coarse-tile slabs, 3 profiled kernels; 6: bin counters on
 * separate 256-B lines of the scratch; 7: + dirt_rasterise_fwd_gbuffer; 8: + dirt_rasterise_bwd_recompute,
 * dirt_bwd_recompute_workspace_size; 9: + the fused lighting helpers dirt_vertex_normals_*,
 * dirt_diffuse_directional_*, dirt_specular_directional_*, dirt_diffuse_point_*; 10: + dirt_stream_capture_id;
 * 11: + dirt_rasterise_fwd_stash, the recompute workspace grows by the gradient stash; 12: the Gouraud forward
 * picks the occluder culling by itself (DIRT_FWD_DEEP_CULL forces it, + DIRT_FWD_DEEP_CULL_OFF); 13: +
 * dirt_rasterise_fwd_resolve; added at 13 without a bump, no signature or layout changed: dirt_dilate_fwd,
 * dirt_dilate_bwd, dirt_deferred_shade_fwd, dirt_deferred_shade_bwd, dirt_texture_sample_fwd,
 * dirt_texture_sample_bwd, dirt_texture_mip_layout, dirt_texture_mip_build_fwd, dirt_texture_mip_build_bwd,
 * dirt_texture_sample_mip_fwd, dirt_texture_sample_mip_bwd, dirt_deferred_shade_lights_workspace,
 * dirt_deferred_shade_lights_fwd, dirt_deferred_shade_lights_bwd, dirt_deferred_shade_sh_workspace,
 * dirt_deferred_shade_sh_fwd, dirt_deferred_shade_sh_bwd, dirt_texture_sample_cube_fwd,
 * dirt_texture_sample_cube_bwd, dirt_texture_sample_cube_mip_fwd, dirt_texture_sample_cube_mip_bwd,
 * dirt_shadow_sample_workspace, dirt_shadow_sample_fwd, dirt_shadow_sample_bwd, dirt_deferred_shade_pbr_workspace,
 * dirt_deferred_shade_pbr_fwd, dirt_deferred_shade_pbr_bwd, dirt_deferred_reflect_view_workspace,
 * dirt_deferred_reflect_view_fwd, dirt_deferred_reflect_view_bwd, dirt_deferred_shade_env_workspace,
 * dirt_deferred_shade_env_fwd, dirt_deferred_shade_env_bwd) */
int dirt_abi_version(void);

/* Byte sizes of the caller-provided buffers for one call.
 * bin_capacity = number of (coarse tile, triangle) bin entries the scratch can hold, split evenly into
 * one slab per (frame, coarse tile); <=0: default policy (F + F/4 + 64 entries per slab, so no slab of
 * a frame overflows unless many faces are clipped into one tile, up to 2^29 entries (4 GiB) in all).  A slab
 * that overflows is still rendered exactly, by a slow path that filters every record of the frame. */
int dirt_workspace_sizes(int B, int H, int W, int C, int V, int F, int64_t bin_capacity,
                         size_t *saved_bytes, size_t *scratch_bytes);

/* Forward: pixels = Rasterise(background, vertices, vertex_colors, faces).
 * gbuffer [B,H,W] int32 receives the per-pixel visible setup-record index (-1 = background),
 * which together with `saved` is what dirt_rasterise_bwd consumes.
 * camera_pos: device pointer to >= 8 floats (9 for DIRT_SHADER_OCEANIC_STILL_CLOUD, 16 for
 * DIRT_SHADER_OCEANIC_OPT_FLOW, 12 for DIRT_SHADER_HILL), used only by the procedural programs
 * (shader_id != 0; may be NULL for Gouraud).  DIRT_SHADER_HILL here reads `background` as a C-channel
 * terrain lookup; dirt_hill_fwd takes one with its own channel count. */
int dirt_rasterise_fwd(const float *background, const float *vertices, const float *vertex_colors,
                       const int32_t *faces, const float *camera_pos,
                       int B, int H, int W, int C, int V, int F, int shader_id,
                       float *pixels, int32_t *gbuffer,
                       void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes,
                       int64_t bin_capacity, unsigned flags,
                       float *zero_grad_vertices, float *zero_grad_vertex_colors, void *stream);
/* Forward with the deferred-shading G-buffer (Gouraud program): dirt_rasterise_fwd plus, per pixel,
 *   depth        [B,H,W]   window depth as the reference's DEPTH24 buffer holds it (rasterise_egl.cpp:248),
 *                          read back as float: d / (2^24 - 1); 1.0 (the clear value, :449) where uncovered
 *   barycentrics [B,H,W,3] perspective-correct barycentrics of the visible face's vertices
 *                          faces[b, face_ids, 0..2] (the `smooth` interpolation, shaders.cpp:16-34); 0 uncovered
 *   face_ids     [B,H,W]   index of the visible face, -1 uncovered
 * (rows top first, like pixels).  Each may be NULL.  Replaces upstream DIRT's G-buffer programs
 * backward_vertex / backward_fragment (csrc/shaders.cpp:2187-2221: barycentrics, 1/gl_FragCoord.w and the
 * face's vertex indices) and the Vertex layout of csrc/rasterise_grad_common.h:5-11. */
int dirt_rasterise_fwd_gbuffer(const float *background, const float *vertices, const float *vertex_colors,
                               const int32_t *faces, int B, int H, int W, int C, int V, int F,
                               float *pixels, int32_t *gbuffer, void *saved, size_t saved_bytes,
                               void *scratch, size_t scratch_bytes, int64_t bin_capacity, unsigned flags,
                               float *zero_grad_vertices, float *zero_grad_vertex_colors,
                               float *depth, float *barycentrics, int32_t *face_ids, void *stream);
/* Forward of a render that shares its geometry with an earlier one (ABI 13): the same vertices, faces, B, H, W and
 * default bin capacity as the Gouraud dirt_rasterise_fwd that wrote `gbuffer_in` and `saved`, other vertex colours
 * [B,V,C] and background [B,H,W,C] (C may differ from that forward's).  Only the resolve runs -- per pixel the visible
 * record from gbuffer_in, its perspective-correct barycentrics from saved, the Gouraud colour of these vertex colours
 * or this background -- so the pixels are bit-identical to a dirt_rasterise_fwd of the same inputs, whose coverage
 * and depth depend on the geometry only.  `gbuffer` [B,H,W] receives this render's copy of the g-buffer (the same
 * words); gbuffer_in and saved are only read, and the later dirt_rasterise_bwd of this render takes `gbuffer` and the
 * same `saved`.  zero_grad_*: as dirt_rasterise_fwd (zero-filled in passing).  samples/deferred.py:63-83 renders
 * one geometry three times (positions, albedo, normals). */
int dirt_rasterise_fwd_resolve(const float *background, const float *vertex_colors, int B, int H, int W, int C, int V,
                               int F, const int32_t *gbuffer_in, const void *saved, size_t saved_bytes, float *pixels,
                               int32_t *gbuffer, float *zero_grad_vertices, float *zero_grad_vertex_colors,
                               void *stream);
/* Forward of the Hill op (csrc/hill.cpp:282-498, REGISTER_OP("Hill") :33-53): DIRT_SHADER_HILL with a
 * terrain lookup `terrain` [B,H,W,terrain_channels] (1, 3 or 4 channels, uploaded like a background,
 * rasterise_egl.cu:33-47) in place of the background; vertex colours are not read.  pixels [B,H,W,C];
 * gbuffer / saved / scratch as dirt_rasterise_fwd (same dirt_workspace_sizes). */
int dirt_hill_fwd(const float *terrain, int terrain_channels, const float *vertices, const int32_t *faces,
                  const float *camera_pos, int B, int H, int W, int C, int V, int F,
                  float *pixels, int32_t *gbuffer, void *saved, size_t saved_bytes, void *scratch,
                  size_t scratch_bytes, int64_t bin_capacity, void *stream);
/* flags of dirt_rasterise_fwd.  Every forward leaves the scratch ready for the next one (the bin counts
 * alternate between two sets, each zeroed by the forward that does not use it), so a scratch buffer that
 * was zero-filled once (or passed to dirt_scratch_clear) and since used only by forwards with the same
 * B, H, W, F and bin_capacity is "clean". */
#define DIRT_FWD_SCRATCH_CLEAN 1u /* the scratch is clean: skip the forward's own clearing memset */
#define DIRT_FWD_DEEP_CULL 2u     /* Gouraud: occluder culling of long per-tile triangle lists before they are
                                     rasterised -- for deep scenes (large overlapping triangles: depth complexity
                                     ~45 at r = 64 px, raster -15 %); results are identical either way, and
                                     scenes of small triangles run slightly faster without it.  Since ABI 12 the
                                     binned Gouraud forward chooses it by itself: each launch counts its long
                                     per-wave lists, and a device takes the culling raster while one of its last
                                     8 forwards was deep (env DIRT_DEEP_CULL_AUTO=0 turns the rule off); this
                                     flag forces it */
#define DIRT_FWD_DEEP_CULL_OFF 8u /* Gouraud: never the occluder culling (the plain raster, as before ABI 12) */
/* zero_grad_vertices [B,V,4] / zero_grad_vertex_colors [B,V,C] (each may be NULL): accumulators the
 * forward zero-fills in passing (filler workgroups of its setup launch, idle CUs), for a later dirt_rasterise_bwd with
 * DIRT_BWD_ACCUMULATE -- a fixed-shape training loop then pays no separate clearing launch.
 * Alignment: no pointer argument of this ABI needs more than its element's natural alignment (4 B);
 * 16-B aligned buffers (every torch / hipMalloc allocation) take the vectorised zero-fill path, others
 * (views at an offset) a scalar one. */

/* Backward: given grad_pixels = dL/dpixels, writes dL/dvertices [B,V,4] (z component is 0),
 * dL/dvertex_colors [B,V,C] and dL/dbackground [B,H,W,C].  All three outputs are fully
 * overwritten (see DIRT_BWD_ACCUMULATE).  grad_background may be NULL when the caller needs no background
 * gradient (a constant background: 4 C bytes per pixel not written); so may one of grad_vertices and
 * grad_vertex_colors (that gradient is then not computed at all: ~30 % less backward time at config 4).  Filter-based (DIRT/OpenDR) derivative,
 * DESIGN.md section 4. */
int dirt_rasterise_bwd(const float *vertices, const float *vertex_colors, const int32_t *faces,
                       const float *pixels, const float *grad_pixels, const int32_t *gbuffer,
                       const void *saved,
                       int B, int H, int W, int C, int V, int F,
                       float *grad_vertices, float *grad_vertex_colors, float *grad_background,
                       unsigned flags, void *stream);
/* flags of dirt_rasterise_bwd */
#define DIRT_BWD_ACCUMULATE 1u /* add into grad_vertices / grad_vertex_colors instead of overwriting them
                                  (e.g. zeroed by the caller on a side stream, off the critical path);
                                  grad_background is always overwritten */
/* Backward of the single-output op: the registered gradient of `Rasterise` computed from the op's own inputs,
 * its output and grad_pixels only -- nothing kept from the forward, so the TensorFlow op stays
 * single-output (csrc/rasterise_egl.cpp:33-53; dirt/rasterise_ops.py:50-54 indexes `[0]`).  Replaces upstream
 * DIRT's gradient path, which re-derived its G-buffer from the op's inputs: launch_vertex_upload +
 * launch_grad_assembly(grad_vertices, grad_vertex_colors, grad_background, ..., pixels, grad_pixels,
 * vertices, ...) (csrc/rasterise_grad_common.h:5-24, declared only in the fork).  Recomputes setup, binning
 * and a coverage-only raster pass (g-buffer + neighbour-coverage bits, bit-identical to the forward's) into
 * `workspace`, then runs the backward kernel of dirt_rasterise_bwd: the same gradients (up to float-atomic
 * summation order), at the cost of the forward's setup and a raster pass without pixel traffic.
 * `pixels` must be the op's output for these inputs.  background / vertex_colors are part of the gradient's
 * inputs and are not read.  Outputs as dirt_rasterise_bwd (fully overwritten unless DIRT_BWD_ACCUMULATE).
 * workspace: caller-owned device memory of dirt_bwd_recompute_workspace_size() bytes; no state survives the
 * call unless DIRT_BWD_SCRATCH_CLEAN is used. */
int dirt_bwd_recompute_workspace_size(int B, int H, int W, int C, int V, int F, size_t *workspace_bytes);
int dirt_rasterise_bwd_recompute(const float *background, const float *vertices, const float *vertex_colors,
                                 const int32_t *faces, const float *pixels, const float *grad_pixels,
                                 int B, int H, int W, int C, int V, int F,
                                 float *grad_vertices, float *grad_vertex_colors, float *grad_background,
                                 void *workspace, size_t workspace_bytes, unsigned flags, void *stream);
/* flags of dirt_rasterise_bwd_recompute: DIRT_BWD_ACCUMULATE, and */
#define DIRT_BWD_SCRATCH_CLEAN 2u /* the workspace was zero-filled once and since used only by recompute
                                     backwards and forward-stashes of the same B, H, W, V, F: skip the bin-counter
                                     memset, and keep the gradient stash */
/* Gradient stash (v11).  The workspace also records the geometry (vertices and faces, bitwise) whose setup records,
 * g-buffer and coverage bits it holds.  dirt_rasterise_bwd_recompute first compares its vertices and faces with that
 * record on the device: when they are identical it skips the recomputation (device-side: the setup and coverage
 * launches exit at once) and runs the backward kernel on what the workspace holds -- the same gradients, since those
 * intermediates are a deterministic function of the geometry and the frame size.  Otherwise it recomputes, and
 * records the new geometry.  dirt_rasterise_fwd_stash is the single-output op's forward that fills the stash as it
 * renders (pixels only as output; background / vertex colours do not enter the stash), so the gradient of that
 * forward costs only the comparison: a TensorFlow kernel pair would share the workspace through a per-device
 * resource keyed by the layout.  A different geometry in between (another render of the same layout) costs one
 * recomputation, never a wrong gradient.  workspace: dirt_bwd_recompute_workspace_size() bytes; flags:
 * DIRT_FWD_SCRATCH_CLEAN when the workspace is clean as DIRT_BWD_SCRATCH_CLEAN describes. */
int dirt_rasterise_fwd_stash(const float *background, const float *vertices, const float *vertex_colors,
                             const int32_t *faces, int B, int H, int W, int C, int V, int F, float *pixels,
                             void *workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* Zero the bin counters of `scratch` for the next forward with the same B, H, W, F, bin_capacity
 * (an async memset of a few KB; lets a caller clear them on another stream, see DIRT_FWD_SCRATCH_CLEAN). */
int dirt_scratch_clear(int B, int H, int W, int F, int64_t bin_capacity, void *scratch, size_t scratch_bytes,
                       void *stream);

/* The id of the HIP graph capture `stream` is recording (hipStreamGetCaptureInfo), 0 when it records none.
 * A scratch created and cleared inside one capture is clean only for that graph's own replays (its clearing
 * memset runs when the graph replays), so callers that cache scratch per stream key it by this id too. */
int dirt_stream_capture_id(void *stream, unsigned long long *capture_id);

/* Debug check (synchronises `stream`): returns DIRT_EFACE if any face index is outside [0,V).  Uses the
 * first 4 bytes of `scratch` as its flag: pass a scratch that no forward is using, or clear it after. */
int dirt_check_faces(const int32_t *faces, int B, int V, int F, void *scratch, size_t scratch_bytes, void *stream);

/* Optional per-kernel timing with HIP events around every launch (used by bench.py for the roofline).
 * dirt_profile_enable(1) clears and starts recording, (0) clears and stops.  dirt_profile_read
 * synchronises the recorded events of kernel `kernel_id` (0..DIRT_NUM_KERNELS-1) and returns its name,
 * launch count and summed duration.  Not thread-safe; do not enable during hipGraph capture. */
#define DIRT_NUM_KERNELS 3
int dirt_profile_enable(int enable);
int dirt_profile_read(int kernel_id, const char **name, int *launches, double *total_ms);

/* Fused lighting helpers: dirt/lighting.py's vertex_normals (:34-98), diffuse_directional (:182-225),
 * specular_directional (:228-288) and diffuse_point (:291-344) -- TensorFlow compositions in the reference (no op of librasterise.so), one
 * kernel per forward / backward here (the deferred-shading chain of samples/deferred.py:62-118 runs them per
 * pixel).  Formulas: dirt_amd/lighting.py.  Light parameters are DEVICE pointers to 3 floats; gradients with
 * respect to them are not computed (the Python layer uses its framework-op statement when they are needed).
 * Backward rules at the kinks as the framework's: d|x| = sign(x) (0 at 0), max(x, 0) passes where x >= 0.
 *
 * vertex_normals: vertices [B,V,vertex_stride] (x, y, z first; stride >= 3), faces [F,3] shared by the B
 * frames (int32, or int64 when faces_int64), out-of-range faces skipped.  summed [B,V,3] (zeroed by the call)
 * is the unnormalised sum the backward needs; normals [B,V,3].  The sums use float atomics: the result may
 * differ in the last bit between calls (as the framework's index_add on a GPU).
 * The backward zero-fills grad_vertices [B,V,grad_stride] and accumulates into its first 3 components;
 * grad_summed [B,V,3] is scratch. */
int dirt_vertex_normals_fwd(const float *vertices, int vertex_stride, const void *faces, int faces_int64, int B, int V,
                            int F, float *summed, float *normals, void *stream);
int dirt_vertex_normals_bwd(const float *vertices, int vertex_stride, const void *faces, int faces_int64, int B, int V,
                            int F, const float *summed, const float *grad_normals, float *grad_summed,
                            float *grad_vertices, int grad_stride, void *stream);
/* diffuse_directional: normals, colors, out [N,3]; out = light_color * colors * clamp(normals . -light_direction).
 * Backward: grad_normals / grad_colors [N,3] overwritten (either may be NULL). */
int dirt_diffuse_directional_fwd(const float *normals, const float *colors, int64_t N, const float *light_direction,
                                 const float *light_color, int double_sided, float *out, void *stream);
int dirt_diffuse_directional_bwd(const float *normals, const float *colors, int64_t N, const float *light_direction,
                                 const float *light_color, int double_sided, const float *grad_out,
                                 float *grad_normals, float *grad_colors, void *stream);
/* diffuse_point: positions, normals, colors, out [N,3]; out = light_color * colors * clamp(normals . unit(positions -
 * light_position)).  Backward: grad_positions / grad_normals / grad_colors [N,3] overwritten (each may be NULL). */
int dirt_diffuse_point_fwd(const float *positions, const float *normals, const float *colors, int64_t N,
                           const float *light_position, const float *light_color, int double_sided, float *out,
                           void *stream);
int dirt_diffuse_point_bwd(const float *positions, const float *normals, const float *colors, int64_t N,
                           const float *light_position, const float *light_color, int double_sided,
                           const float *grad_out, float *grad_positions, float *grad_normals, float *grad_colors,
                           void *stream);
/* specular_directional: positions, normals, reflectivities, out [N,3]; Phong lobe around the reflected light
 * direction, out = light_color * reflectivities * clamp(cos)^shininess.  Backward: the three input gradients
 * [N,3] overwritten (each may be NULL). */
int dirt_specular_directional_fwd(const float *positions, const float *normals, const float *reflectivities, int64_t N,
                                  const float *light_direction, const float *light_color,
                                  const float *camera_position, float shininess, int double_sided, float *out,
                                  void *stream);
int dirt_specular_directional_bwd(const float *positions, const float *normals, const float *reflectivities, int64_t N,
                                  const float *light_direction, const float *light_color,
                                  const float *camera_position, float shininess, int double_sided,
                                  const float *grad_out, float *grad_positions, float *grad_normals,
                                  float *grad_reflectivities, void *stream);

/* Deferred shading in pixel space (samples/deferred.py:85-115): silhouette dilation and the fused G-buffer lighting.
 * One launch per call; the backwards are gathers in a fixed order (no float atomics), so their gradients are
 * bit-identical from run to run.  H, W in 1..DIRT_MAX_DIM, C in 1..DIRT_MAX_CHANNELS, B >= 0 (B == 0: no-op).
 *
 * dilate: x, out [B,H,W,C]; mask [B,H,W] uint8, NULL = "any channel of x[p] is +inf or -inf".
 *   out[p,c] = mask[p] ? max of x[.,c] over the 3x3 window around p clipped to its frame : x[p,c]
 * The max scans the window in row-major order from its first element and replaces the running value when
 * v > m || isnan(v) (the framework's CPU max_pool2d): the first maximum wins ties, a NaN in the window gives NaN
 * (the last one wins), an all -inf window picks its first element.  route [B,H,W] receives a 4-bit code per channel
 * from bit 0: 0..8 = the winner's window position (dy + 1) * 3 + (dx + 1), 15 = not dilated (unused nibbles 0).
 * Backward, from grad_out and route alone:
 *   grad_x[p,c] = (code(p,c) == 15 ? grad_out[p,c] : 0) + the grad_out[q,c] of the window positions q around p, in
 *   row-major order and including p itself, whose code for c points back at p.
 * out / grad_x must not alias x / grad_out. */
int dirt_dilate_fwd(const float *x, const uint8_t *mask, int B, int H, int W, int C, float *out, uint32_t *route,
                    void *stream);
int dirt_dilate_bwd(const float *grad_out, const uint32_t *route, int B, int H, int W, int C, float *grad_x,
                    void *stream);
/* deferred_shade: positions, colors, normals, pixels [B,H,W,3]; the five light parameters are DEVICE pointers to 3
 * floats (no gradient with respect to them).  Per pixel: bg = any channel of positions[p] is +-inf; positions and
 * normals are dilated as above, both under bg; valid = all six dilated values are finite;
 *   pixels = valid ? (diffuse_directional(normals_d, colors) + specular_directional(positions_d, normals_d, colors))
 *                    + colors * ambient_color : 0
 * (both lights one direction, the fused lighting helpers' arithmetic).  valid [B,H,W] uint8; route [B,H,W]: the
 * positions' codes in bits 0..11, the normals' in bits 12..23, valid in bit 31.
 * Backward: grad_positions / grad_colors / grad_normals [B,H,W,3], each fully overwritten, each may be NULL; the
 * lighting adjoints (zero at invalid pixels) routed through the dilation by the gather above. */
int dirt_deferred_shade_fwd(const float *positions, const float *colors, const float *normals, int B, int H, int W,
                            const float *ambient_color, const float *light_direction, const float *diffuse_color,
                            const float *specular_color, const float *camera_position, float shininess,
                            int double_sided, float *pixels, uint8_t *valid, uint32_t *route, void *stream);
int dirt_deferred_shade_bwd(const float *positions, const float *colors, const float *normals, int B, int H, int W,
                            const float *ambient_color, const float *light_direction, const float *diffuse_color,
                            const float *specular_color, const float *camera_position, float shininess,
                            int double_sided, const float *grad_pixels, const uint32_t *route, float *grad_positions,
                            float *grad_colors, float *grad_normals, void *stream);

/* deferred_shade_lights: deferred_shade under n_lights lights (0..DIRT_MAX_LIGHTS; 0 = ambient only), with gradients
 * to the light parameters.  Dilation, valid and the route word are deferred_shade's.  Bit i of point_mask makes light
 * i a point light (bits at or above n_lights must be clear).  light_vectors, diffuse_colors, specular_colors are
 * DEVICE arrays [n_lights,3] shared by the frames, or [B,n_lights,3] with lights_per_frame != 0; camera_position is
 * [3], or [B,3] with camera_per_frame != 0; ambient_color is 3 floats shared by the frames, NULL = zero; the
 * shininess is read from the device through shininess_ptr when that is not NULL, else it is shininess_value.  Nothing
 * is copied from the host per call: the calls can be captured into a graph.  For a valid pixel, lights in index order:
 *   acc = (d_0 + s_0);  acc = acc + (d_i + s_i);  pixels = acc + colors * ambient_color
 *   directional light, row l (used raw): d = diffuse_directional, s = specular_directional, colours as reflectivities
 *   point light, row = its position: u = (p - light) / (|p - light| + 1e-12); d = diffuse_point; s =
 *   specular_directional with u in place of the direction (the gradient flows through u into p and the light's
 *   position); no distance attenuation.
 * Backward: grad_positions / grad_colors / grad_normals as deferred_shade_bwd's; grad_ambient [3], grad_light_vectors,
 * grad_diffuse_colors, grad_specular_colors, grad_camera (shaped as their parameters) and grad_shininess [1] receive
 * the sums of the per-pixel terms over the valid pixels of a frame (per-frame parameters) or of all frames (shared
 * ones).  Each of the nine may be NULL; each requested one is fully overwritten.  With a parameter gradient
 * requested, `workspace` must hold dirt_deferred_shade_lights_workspace() bytes (it needs no clearing): the first
 * kernel stores per-chunk partial sums [B][chunks][7 + 9 n_lights] there -- one workgroup per 256 contiguous pixels
 * of a frame, wave butterflies, then the four waves in order -- and a second kernel on the same stream adds the
 * chunks of a frame and then the frames in fixed orders.  No float atomics: every gradient is bit-identical from run
 * to run.  B == 0, or nothing requested, is DIRT_OK without a launch. */
#define DIRT_MAX_LIGHTS 8
int dirt_deferred_shade_lights_workspace(int B, int H, int W, int n_lights, size_t *bytes);
int dirt_deferred_shade_lights_fwd(const float *positions, const float *colors, const float *normals, int B, int H,
                                   int W, const float *ambient_color, int n_lights, unsigned point_mask,
                                   int lights_per_frame, const float *light_vectors, const float *diffuse_colors,
                                   const float *specular_colors, int camera_per_frame, const float *camera_position,
                                   float shininess_value, const float *shininess_ptr, int double_sided, float *pixels,
                                   uint8_t *valid, uint32_t *route, void *stream);
int dirt_deferred_shade_lights_bwd(const float *positions, const float *colors, const float *normals, int B, int H,
                                   int W, const float *ambient_color, int n_lights, unsigned point_mask,
                                   int lights_per_frame, const float *light_vectors, const float *diffuse_colors,
                                   const float *specular_colors, int camera_per_frame, const float *camera_position,
                                   float shininess_value, const float *shininess_ptr, int double_sided,
                                   const float *grad_pixels, const uint32_t *route, float *grad_positions,
                                   float *grad_colors, float *grad_normals, float *grad_ambient,
                                   float *grad_light_vectors, float *grad_diffuse_colors, float *grad_specular_colors,
                                   float *grad_camera, float *grad_shininess, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* deferred_shade_pbr: the metallic-roughness model (Lambert plus a GGX microfacet lobe) under n_lights lights
 * (0..DIRT_MAX_LIGHTS; 0 = ambient only) with a per-pixel, per-light visibility, and gradients to every input.
 * Dilation of positions and normals, valid and the route word are deferred_shade's; colors (the base colour), material
 * [B,H,W,2] (perceptual roughness, metallic) and visibility [B,H,W,n_lights] (NULL = ones) are read at the pixel
 * itself.  The light arrays, the camera, the ambient colour and point_mask are deferred_shade_lights': DEVICE arrays
 * [n_lights,3] or [B,n_lights,3], [3] or [B,3], 3 floats or NULL; a directional light's row is its direction of
 * travel, a point light's row its position.  For a valid pixel with dilated position p, dilated normal n_d, colour c,
 * u(x) = x / (|x| + 1e-12):
 *   n = u(n_d)  v = u(camera - p)  l = u(-direction) or u(position - p)  h = u(l + v)
 *   r = clamp(material_0, DIRT_PBR_MIN_ROUGHNESS, 1)  m = clamp(material_1, 0, 1)  alpha = r r  k = alpha / 2
 *   nl = n . l  nv = max(n . v, 0)  nh = n . h  vh = clamp(v . h, 0, 1)
 *   t = |n x h|^2 + (nh alpha)^2   D = t > 0 ? alpha^2 / (pi t^2) : 0   V = 1 / (4 (nl (1 - k) + k) (nv (1 - k) + k))
 *   F0 = 0.04 + (c - 0.04) m   F = F0 + (1 - F0) (1 - vh)^5
 *   term_i = nl > 0 ? visibility_i (light_color_i nl) ((1 - F) (1 - m) c / pi + D V F) : 0   (no attenuation)
 *   pixels = term_0 + term_1 + ... + c * ambient_color, 0 at an invalid pixel.
 * Backward: grad_positions / grad_normals are gathers through the dilation route as deferred_shade_bwd's; grad_colors,
 * grad_material, grad_visibility receive their own pixel's terms (every clamp with torch.clamp's derivative, the two
 * selects with none on their zero side); grad_ambient [3], grad_light_vectors, grad_light_colors, grad_camera (shaped
 * as their parameters) receive the sums of the per-pixel terms over the valid pixels of a frame (per-frame parameters)
 * or of all frames (shared ones).  Each of the nine may be NULL; each requested one is fully overwritten.  With a
 * parameter gradient requested, `workspace` must hold dirt_deferred_shade_pbr_workspace() bytes = B * ceil(H W / 256)
 * * (6 + 6 n_lights) * 4 (it needs no clearing): the first kernel stores per-chunk partial sums there -- one workgroup
 * per 256 contiguous pixels of a frame, wave butterflies, then the four waves in order -- and a second kernel on the
 * same stream adds the chunks of a frame and then the frames in fixed orders.  No float atomics: every gradient is
 * bit-identical from run to run.  B == 0, or nothing requested, is DIRT_OK without a launch. */
#define DIRT_PBR_MIN_ROUGHNESS 0.045f
int dirt_deferred_shade_pbr_workspace(int B, int H, int W, int n_lights, size_t *bytes);
int dirt_deferred_shade_pbr_fwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *visibility, int B, int H, int W,
                                const float *ambient_color, int n_lights, unsigned point_mask, int lights_per_frame,
                                const float *light_vectors, const float *light_colors, int camera_per_frame,
                                const float *camera_position, float *pixels, uint8_t *valid, uint32_t *route,
                                void *stream);
int dirt_deferred_shade_pbr_bwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *visibility, int B, int H, int W,
                                const float *ambient_color, int n_lights, unsigned point_mask, int lights_per_frame,
                                const float *light_vectors, const float *light_colors, int camera_per_frame,
                                const float *camera_position, const float *grad_pixels, const uint32_t *route,
                                float *grad_positions, float *grad_colors, float *grad_normals, float *grad_material,
                                float *grad_visibility, float *grad_ambient, float *grad_light_vectors,
                                float *grad_light_colors, float *grad_camera, void *workspace, size_t workspace_bytes,
                                void *stream);

/* deferred_shade_sh: the colour G-buffer lit by low-order spherical harmonics of the normal G-buffer, with gradients
 * to both G-buffers and to the coefficients.  colors, normals, pixels [B,H,W,3]; mask [B,H,W] uint8, NULL = "any
 * channel of normals[p] is +inf or -inf" (dilate's default).  normals are dilated under mask by dilate's rule; valid
 * [B,H,W] uint8 = the three dilated values are finite; route [B,H,W]: the normals' three codes from bit 0 in dilate's
 * layout, valid in bit 31 (the backward needs no mask).  coefficients is a DEVICE array [n_coeffs,3] shared by the
 * frames, or [B,n_coeffs,3] with coeffs_per_frame != 0; n_coeffs is 1, 4 or 9 (bands 0, 0-1, 0-2).  Nothing is copied
 * from the host per call: the calls can be captured into a graph.  With normalize != 0 the dilated normal n is
 * replaced by u = n / (|n| + 1e-12) (diffuse_point's rule), else it is used raw.  For a valid pixel, (x, y, z) that
 * vector, float32, every step one IEEE operation, the constants the float32 roundings of
 *   c0 = 0.28209479177387814  c1 = 0.4886025119029199  c2 = 1.0925484305920792  c3 = 0.31539156525252005
 *   c4 = 0.5462742152960396:
 *   Y0 = c0          Y1 = c1 y        Y2 = c1 z            Y3 = c1 x
 *   Y4 = c2 (x y)    Y5 = c2 (y z)    Y6 = c3 (3 z^2 - 1)  Y7 = c2 (x z)    Y8 = c4 (x^2 - y^2)
 *   E_c = coefficients[0,c] Y0;  E_c = E_c + coefficients[k,c] Y_k for k = 1 .. n_coeffs - 1 in index order
 *   pixels_c = colors_c E_c
 * and pixels = 0 at an invalid pixel.  There is no clamp (an irradiance may be negative), and the cosine-lobe factors
 * (pi, 2 pi / 3, pi / 4) are the caller's to fold into the coefficients.
 * Backward, g = grad_pixels at valid pixels and 0 elsewhere: grad_colors_c = g_c E_c; with gE_c = g_c colors_c,
 * grad_coefficients[k,c] = the sum of gE_c Y_k over the valid pixels of the frame (per-frame form) or of all frames
 * (shared form); the normal's adjoint g_u = sum_c gE_c sum_k coefficients[k,c] grad Y_k -- with normalize passed
 * through J = I / d - h h^T |n| / d^2, d = |n| + 1e-12, h = n / |n| (0 at n = 0) -- is routed through the dilation by
 * dilate's gather into grad_normals.  Each of the three may be NULL; each requested one is fully overwritten.  With
 * grad_coefficients requested, `workspace` must hold dirt_deferred_shade_sh_workspace() bytes = B * ceil(H W / 256) *
 * 3 n_coeffs * 4 (it needs no clearing): the first kernel stores per-chunk partial sums [B][chunks][3 n_coeffs] there
 * -- one workgroup per 256 contiguous pixels of a frame, wave butterflies, then the four waves in order -- and a second
 * kernel on the same stream adds the chunks of a frame and then the frames in fixed orders.  No float atomics: every
 * gradient is bit-identical from run to run.  B == 0, or nothing requested, is DIRT_OK without a launch. */
#define DIRT_MAX_SH_COEFFS 9
int dirt_deferred_shade_sh_workspace(int B, int H, int W, int n_coeffs, size_t *bytes);
int dirt_deferred_shade_sh_fwd(const float *colors, const float *normals, const uint8_t *mask, int B, int H, int W,
                               int n_coeffs, int coeffs_per_frame, const float *coefficients, int normalize,
                               float *pixels, uint8_t *valid, uint32_t *route, void *stream);
int dirt_deferred_shade_sh_bwd(const float *colors, const float *normals, int B, int H, int W, int n_coeffs,
                               int coeffs_per_frame, const float *coefficients, int normalize,
                               const float *grad_pixels, const uint32_t *route, float *grad_colors,
                               float *grad_normals, float *grad_coefficients, void *workspace,
                               size_t workspace_bytes, void *stream);

/* Image-based lighting: the two steps between deferred_shade_sh, texture_sample_cube_mip and deferred_shade_pbr.
 * Dilation of positions and normals under the positions' background, valid and the route word are deferred_shade's;
 * camera_position is a DEVICE array [3], or [B,3] with camera_per_frame != 0.  u(x) = x / (|x| + 1e-12).
 *
 * deferred_reflect_view: the reflection of the view vector about the normal, directions [B,H,W,3].  For a valid pixel
 * with dilated position p and dilated normal n_d, float32, every step one IEEE operation:
 *   n = u(n_d)  v = u(camera - p)  nvr = n . v (not clamped)  t = 2 nvr  R = t n - v
 * and exactly (0, 0, 0) at an invalid pixel, a direction both cube-map lookups leave out.
 *
 * deferred_shade_env: the split-sum combination of a diffuse irradiance environment (coefficients: deferred_shade_sh's
 * basis, order and constants; [n_coeffs,3], or [B,n_coeffs,3] with coeffs_per_frame != 0; n_coeffs 1, 4 or 9) and a
 * prefiltered specular one (radiance [B,H,W,3]).  colors, material [B,H,W,2] (perceptual roughness, metallic), radiance
 * and occlusion [B,H,W] (NULL = ones) are read at the pixel itself.  For a valid pixel with colour c:
 *   n = u(n_d)  v = u(camera - p)  nv = max(n . v, 0)
 *   r = clamp(material_0, DIRT_PBR_MIN_ROUGHNESS, 1)  m = clamp(material_1, 0, 1)
 *   E = coefficients_0 Y_0 + coefficients_1 Y_1(n) + ...   (deferred_shade_sh's order of additions)
 *   F0 = 0.04 + (c - 0.04) m
 *   x = 1 - r  y = 0.0425 - 0.0275 r  z = 1.04 - 0.572 r  w = 0.022 r - 0.04
 *   e = exp2(-9.28 nv)  q = x x  s = q < e ? q : e  a = s x + y  A = z - 1.04 a  B = 1.04 a + w
 *   S = F0 A + B  dif = ((1 - m) c) E  spec = radiance S  pixels = occlusion (dif + spec)
 * and 0 at an invalid pixel.  The cosine-lobe factors and any 1 / pi are the caller's to fold into the coefficients.
 *
 * Backward: grad_positions / grad_normals are gathers through the dilation route as deferred_shade_bwd's; grad_colors,
 * grad_material, grad_radiance, grad_occlusion receive their own pixel's terms (every clamp with torch.clamp's
 * derivative, max(., 0) passing where its argument is >= 0, the select passing to its chosen side only);
 * grad_coefficients and grad_camera (shaped as their parameters) receive the sums of the per-pixel terms over the
 * valid pixels of a frame (per-frame parameters) or of all frames (shared ones).  Each may be NULL; each requested one
 * is fully overwritten.  With a parameter gradient requested, `workspace` must hold dirt_deferred_*_workspace() bytes
 * = B * ceil(H W / 256) * P * 4 (it needs no clearing), P = 3 (reflect_view: the camera) or 3 + 3 n_coeffs (shade_env:
 * the camera, then the coefficients in index order): the first kernel stores per-chunk partial sums there -- one
 * workgroup per 256 contiguous pixels of a frame, wave butterflies, then the four waves in order -- and a second kernel
 * on the same stream adds the chunks of a frame and then the frames in fixed orders.  No float atomics: every gradient
 * is bit-identical from run to run.  B == 0, or nothing requested, is DIRT_OK without a launch. */
int dirt_deferred_reflect_view_workspace(int B, int H, int W, size_t *bytes);
int dirt_deferred_reflect_view_fwd(const float *positions, const float *normals, int B, int H, int W,
                                   int camera_per_frame, const float *camera_position, float *directions,
                                   uint8_t *valid, uint32_t *route, void *stream);
int dirt_deferred_reflect_view_bwd(const float *positions, const float *normals, int B, int H, int W,
                                   int camera_per_frame, const float *camera_position, const float *grad_directions,
                                   const uint32_t *route, float *grad_positions, float *grad_normals,
                                   float *grad_camera, void *workspace, size_t workspace_bytes, void *stream);
int dirt_deferred_shade_env_workspace(int B, int H, int W, int n_coeffs, size_t *bytes);
int dirt_deferred_shade_env_fwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *radiance, const float *occlusion, int B, int H,
                                int W, int n_coeffs, int coeffs_per_frame, const float *coefficients,
                                int camera_per_frame, const float *camera_position, float *pixels, uint8_t *valid,
                                uint32_t *route, void *stream);
int dirt_deferred_shade_env_bwd(const float *positions, const float *colors, const float *normals,
                                const float *material, const float *radiance, const float *occlusion, int B, int H,
                                int W, int n_coeffs, int coeffs_per_frame, const float *coefficients,
                                int camera_per_frame, const float *camera_position, const float *grad_pixels,
                                const uint32_t *route, float *grad_positions, float *grad_colors, float *grad_normals,
                                float *grad_material, float *grad_radiance, float *grad_occlusion,
                                float *grad_coefficients, float *grad_camera, void *workspace, size_t workspace_bytes,
                                void *stream);

/* Deferred texturing: bilinear sampling of a texture at a uv G-buffer, and its gradients.
 * texture [texture_frames,Th,Tw,C] (texture_frames = 1: shared by the B frames, = B: one per frame), uv [B,H,W,2],
 * mask [B,H,W] uint8 (NULL = "both uv channels are finite"), texels [B,H,W,C], valid [B,H,W] uint8 (0 / 1).
 * u runs along the texture's width, v along its height, the top row first; texel (i,j) has its centre at
 * u = (j + 0.5) / Tw, v = (i + 0.5) / Th.  H, W, Th, Tw in 1..DIRT_MAX_DIM, C in 1..DIRT_MAX_CHANNELS, B >= 0
 * (B == 0: no-op).  Rule, float32, every step one IEEE operation; for u with T = Tw (v with Th alike):
 *   DIRT_TEXTURE_CLAMP (GL CLAMP_TO_EDGE): uc = min(max(u, 0), 1)      DIRT_TEXTURE_REPEAT: uc = u - floor(u)
 *   x = uc * T;  x = x - 0.5;  fx = floor(x);  a = x - fx;  j0 = (int)fx;  j1 = j0 + 1
 *   j0, j1 reduced into [0, T): clamped, or modulo T in repeat mode (uc may round to exactly 1: j1 = T -> 0)
 * (fx is clamped to [-1, T] and a NaN sent to -1 before the conversion: no uv, finite or not, addresses outside the
 * texture.)  Per channel, each product and sum rounded once in this order:
 *   top = t[i0,j0] * (1 - a) + t[i0,j1] * a;  bot = t[i1,j0] * (1 - a) + t[i1,j1] * a;  out = top * (1 - b) + bot * b
 * Pixels that are not sampled give exactly 0 and valid 0, carry no gradient and form no address.
 * Backward, with g = grad_texels[p,:] at sampled pixels:
 *   grad_texture[i0,j0,c] += g_c * (1 - a) * (1 - b), and likewise for the other three taps;
 *   grad_u = pass_u ? Tw * sum_c g_c * ((t[i0,j1] - t[i0,j0]) * (1 - b) + (t[i1,j1] - t[i1,j0]) * b) : 0
 *   grad_v = pass_v ? Th * sum_c g_c * (bot_c - top_c) : 0;   pass_u: 0 <= u <= 1 (clamp), always (repeat).
 * grad_texture [texture_frames,Th,Tw,C] is zero-filled on `stream` by the call (an asynchronous memset, capturable)
 * and fully overwritten; with texture_frames = 1 it sums over the frames.  It is summed with float atomics: the
 * result may differ in the last bits between calls (as dirt_vertex_normals_*).  grad_uv [B,H,W,2] is fully
 * overwritten, zero at unsampled pixels; it is a gather in a fixed order, bit-identical from run to run.  Either
 * gradient may be NULL; with both NULL the backward returns DIRT_OK without a launch. */
#define DIRT_TEXTURE_CLAMP 0
#define DIRT_TEXTURE_REPEAT 1
int dirt_texture_sample_fwd(const float *texture, int texture_frames, int Th, int Tw, int C, const float *uv,
                            const uint8_t *mask, int B, int H, int W, int wrap, float *texels, uint8_t *valid,
                            void *stream);
int dirt_texture_sample_bwd(const float *texture, int texture_frames, int Th, int Tw, int C, const float *uv,
                            const uint8_t *mask, int B, int H, int W, int wrap, const float *grad_texels,
                            float *grad_texture, float *grad_uv, void *stream);

/* Mipmapped deferred texturing: a box-filtered mip chain of a texture and its trilinear lookup at a uv G-buffer.
 * Chain of a texture [texture_frames,Th,Tw,C]: level 0 is the texture; level k+1 exists while level k has every
 * dimension even or 1 and not both 1, with dimensions max(1, T/2) (an odd dimension > 1 ends the chain: 5x7 has 1
 * level, 6x10 has 2, 64x64 has 7, 8192x8192 has 14 = DIRT_MAX_MIP_LEVELS).  float32, each sum and product rounded once:
 *   both dimensions >= 2:  t'[i,j] = ((t[2i,2j] + t[2i,2j+1]) + (t[2i+1,2j] + t[2i+1,2j+1])) * 0.25
 *   one dimension 1:       t'[j] = (t[2j] + t[2j+1]) * 0.5 along the other.
 * packed [texture_frames,N,C], N = sum_k Th_k * Tw_k: the levels in order, each row-major.  `levels` truncates the
 * chain (<= 0: the whole chain; more than the chain has: DIRT_EINVAL); the same value goes to all four entry points.
 *
 * dirt_texture_mip_layout is host-only (no GPU call): returns the number of levels L for max_levels (<= 0: the whole
 * chain) and writes dims[2k], dims[2k+1] = Th_k, Tw_k, offsets[k] = the first texel of level k inside a frame, and
 * *total = N (each pointer may be NULL; dims holds 2 * DIRT_MAX_MIP_LEVELS ints, offsets DIRT_MAX_MIP_LEVELS).  It
 * returns 0, with a message in dirt_last_error, for dimensions outside 1..DIRT_MAX_DIM.
 *
 * dirt_texture_mip_build_fwd writes every level of packed (level 0 is a copy).  dirt_texture_mip_build_bwd takes
 * grad_packed [texture_frames,N,C] (read only) to grad_texture [texture_frames,Th,Tw,C] (fully overwritten) as one
 * gather per level-0 element in a fixed order, w_k = 0.25 or 0.5 the forward's box weight from level k to k+1:
 *   acc = g[L-1][i >> (L-1), j >> (L-1)];  for k = L-2 .. 0:  acc = acc * w_k + g[k][i >> k, j >> k]
 * (no atomics, no scratch buffer, bit-identical from run to run).  texture_frames == 0 is a no-op.
 *
 * Lookup.  uv [B,H,W,2], mask [B,H,W] uint8 (NULL = "both uv channels are finite"), conventions, limits and the
 * per-level bilinear rule s_k as dirt_texture_sample_* with T = T_k.  Level of detail of a sampled pixel (y,x),
 * float32, every step one IEEE operation, from the raw uv (before any wrap):
 *   x-difference d = uv[y,x+1] - uv[y,x] if x+1 < W and that neighbour is sampled, else uv[y,x] - uv[y,x-1] if
 *   x >= 1 and that neighbour is sampled, else 0; the y-difference alike;
 *   du = d_u * Tw;  dv = d_v * Th;  q = du * du + dv * dv;  rho2 = fmax(qx, qy)  (a NaN loses against a number);
 *   rho2 = m * 2^e, m in [1,2), both from the float's bit fields;  lod = 0.5 * (e + (m - 1));
 *   lod = 0 unless rho2 >= 1 (0, subnormals, NaN);  lod = L-1 when rho2 is inf.
 * lod_in [B,H,W] (nullable) replaces all of that; a NaN in it becomes 0.  Then lod = lod + lod_bias (finite), clamped
 * to [0, L-1].  k0 = (int)floor(lod), f = lod - k0, k1 = min(k0+1, L-1):
 *   out = s_k0 * (1 - f) + s_k1 * f;   f == 0: out = s_k0 and level k1 is not read.
 * texels [B,H,W,C], valid [B,H,W] uint8 (0 / 1) and lod [B,H,W] (each pixel's final lod, 0 where unsampled) are fully
 * overwritten; unsampled pixels give exactly 0 and valid 0, carry no gradient and form no address.
 * THE LOD CARRIES NO GRADIENT, neither to uv nor to lod_in: the backward takes the forward's lod buffer as a constant.
 * Backward, with g = grad_texels[p,:] at sampled pixels:
 *   grad_packed[level k0, tap, c] += g_c * w1 * w2 * (1 - f), grad_packed[level k1, tap, c] += g_c * w1 * w2 * f for
 *   the four taps of each level (w1, w2 the level's bilinear weights; f == 0: the four taps of k0 alone, weight 1);
 *   grad_uv = grad_uv(k0) * (1 - f) + grad_uv(k1) * f, each term dirt_texture_sample_bwd's formula with T_k and its
 *   pass rule (f == 0: grad_uv(k0)).
 * grad_packed [texture_frames,N,C] is zero-filled on `stream` by the call (an asynchronous memset, capturable) and
 * summed with float atomics (last bits may differ between calls); grad_uv [B,H,W,2] is a gather in a fixed order,
 * bit-identical from run to run, zero at unsampled pixels.  Either may be NULL; with both NULL no launch is made.
 * B == 0 is a no-op.  Every argument error is a return code raised before any GPU call. */
#define DIRT_MAX_MIP_LEVELS 14
int dirt_texture_mip_layout(int Th, int Tw, int max_levels, int *dims, long long *offsets, long long *total);
int dirt_texture_mip_build_fwd(const float *texture, int texture_frames, int Th, int Tw, int C, int levels,
                               float *packed, void *stream);
int dirt_texture_mip_build_bwd(const float *grad_packed, int texture_frames, int Th, int Tw, int C, int levels,
                               float *grad_texture, void *stream);
int dirt_texture_sample_mip_fwd(const float *packed, int texture_frames, int Th, int Tw, int C, int levels,
                                const float *uv, const uint8_t *mask, const float *lod_in, float lod_bias, int B, int H,
                                int W, int wrap, float *texels, uint8_t *valid, float *lod, void *stream);
int dirt_texture_sample_mip_bwd(const float *packed, int texture_frames, int Th, int Tw, int C, int levels,
                                const float *uv, const uint8_t *mask, const float *lod, int B, int H, int W, int wrap,
                                const float *grad_texels, float *grad_packed, float *grad_uv, void *stream);

/* Cube-map lookup: bilinear sampling of a cube map at a direction G-buffer, and its gradients.
 * cubemap [cubemap_frames,6,S,S,C] (cubemap_frames = 1: shared by the B frames, = B: one per frame), faces in the order
 * +x, -x, +y, -y, +z, -z, each laid out as a texture of dirt_texture_sample_*; directions [B,H,W,3], any length;
 * mask [B,H,W] uint8 or NULL.  1 <= S <= DIRT_MAX_DIM, 1 <= C <= DIRT_MAX_CHANNELS.  A pixel is sampled where the mask
 * is nonzero (NULL: everywhere) and its direction's three values are finite and not all zero; the others give texels
 * exactly 0 and valid 0, receive gradient 0 and never form an address.  Rule (float32, every line one IEEE operation):
 *   major axis: x if |x| >= |y| && |x| >= |z|, else y if |y| >= |z|, else z; ma = that component; the negative face
 *   exactly when ma < 0;  (sc, tc) = +x: (-z, -y)  -x: (z, -y)  +y: (x, z)  -y: (x, -z)  +z: (x, -y)  -z: (-x, -y)
 *   m = |ma|;  su = sc / m;  sv = tc / m;  u = su + 1;  u = u * 0.5;  v = sv + 1;  v = v * 0.5
 * and the face's texels filtered at (u, v) by dirt_texture_sample_*'s clamp rule with Th = Tw = S: filtering clamps
 * to the face's edge, there is none across face seams.
 * Backward, g = grad_texels[p,:] at sampled pixels: (gu, gv) as dirt_texture_sample_bwd's grad_uv on the face, then
 *   hu = 0.5 * gu;  hv = 0.5 * gv;  g_sc = hu / m;  g_tc = hv / m;  t = hu * su;  t2 = hv * sv;  t = t + t2
 *   g_m = t / m;  g_m = -g_m;  g_ma = ma < 0 ? -g_m : g_m
 * written to grad_directions [B,H,W,3] through the table's signs (fixed order, bit-identical from run to run).
 * grad_cubemap [cubemap_frames,6,S,S,C] is zero-filled on `stream` by the call (an asynchronous memset, capturable)
 * and receives the four-tap scatter of dirt_texture_sample_bwd into the selected face, summed with float atomics.
 * Either gradient pointer may be NULL (not wanted); with both NULL, or B == 0, the call is a no-op. */
int dirt_texture_sample_cube_fwd(const float *cubemap, int cubemap_frames, int S, int C, const float *directions,
                                 const uint8_t *mask, int B, int H, int W, float *texels, uint8_t *valid, void *stream);
int dirt_texture_sample_cube_bwd(const float *cubemap, int cubemap_frames, int S, int C, const float *directions,
                                 const uint8_t *mask, int B, int H, int W, const float *grad_texels,
                                 float *grad_cubemap, float *grad_directions, void *stream);

/* Seamless mip-mapped cube-map lookup: the trilinear lookup of a cube map's mip chain at a direction G-buffer, and its
 * gradients to the chain, the directions and an explicit level of detail.
 * packed [cubemap_frames,6,N,C]: each face's chain as dirt_texture_mip_build_fwd packs it (call that with
 * texture_frames = 6 * cubemap_frames, Th = Tw = S; N = sum_k S_k^2, S_k = S >> k while S_k is even; `levels` as
 * there), or a chain of that layout prefiltered any other way.  directions, mask, the sampled-pixel rule, the limits
 * and face, ma, m, su, sv, u, v as dirt_texture_sample_cube_*.  Rule (float32, every line one IEEE operation):
 *   lod: lod_in [B,H,W] (a NaN counts as 0), or with lod_in NULL from the point P = (x / m, y / m, z / m) on the unit
 *     cube, which is continuous across the seams: the x-difference e = P[y,x+1] - P[y,x] if x+1 < W and that
 *     neighbour is sampled, else P[y,x] - P[y,x-1] if x >= 1 and that neighbour is sampled, else 0; the y-difference
 *     alike;  h = 0.5 * S;  e = e * h per component;  q = ex * ex;  t = ey * ey;  q = q + t;  t = ez * ez;  q = q + t;
 *     rho2 = fmax(qx, qy);  then dirt_texture_sample_mip_*'s tail (lod = 0.5 * (e + (m - 1)) from rho2's bit fields,
 *     0 unless rho2 >= 1, L-1 at inf).
 *   lod = lod + lod_bias (finite), clamped to [0, L-1];  k0 = (int)floor(lod), f = lod - k0, k1 = min(k0+1, L-1).
 *   taps at level k, T = S_k:  x = u * T;  x = x - 0.5;  fx = floor(x);  a = x - fx;  j0 = (int)fx;  j1 = j0 + 1 (so
 *     j0 in [-1, T-1], j1 in [0, T]);  i0, i1, b from v alike.
 *     seamless = 0: the four indices clamped to [0, T-1], dirt_texture_sample_cube_*'s rule at every level.
 *     seamless = 1: tap (i, j) is resolved in integers (GL_TEXTURE_CUBE_MAP_SEAMLESS is the model).  sc = 2j + 1 - T,
 *       tc = 2i + 1 - T, and the inverse face table with major T gives its point:
 *         +x: (T,-tc,-sc)  -x: (-T,-tc,sc)  +y: (sc,T,tc)  -y: (sc,-T,-tc)  +z: (sc,-tc,T)  -z: (-sc,-tc,-T)
 *       both indices in range: texel (i, j) of the pixel's face.  One out of range (one coordinate of magnitude T+1):
 *       that coordinate becomes +-T and the major axis, the old major coordinate +-(T-1), the third stays; the face
 *       table gives (face', sc', tc') and j' = (sc' + T - 1) / 2, i' = (tc' + T - 1) / 2, exact integers in [0, T).
 *       Both out of range (a cube corner, at most one of the four taps): no texel exists; the tap's value is
 *       ((t_p + t_q) + t_r) * third, third = float32(1/3), p, q, r the other three taps in the order 00, 01, 10, 11.
 *   s_k = the bilinear rule's three lines on the four tap values;  out = s_k0 * (1 - f) + s_k1 * f;  f == 0:
 *   out = s_k0 and level k1 is not read.
 * texels [B,H,W,C], valid [B,H,W] uint8 (0 / 1) and lod [B,H,W] (each pixel's final lod, 0 where unsampled) are fully
 * overwritten.
 * Backward, with g = grad_texels[p,:] at sampled pixels; lod is the forward's buffer, lod_in and lod_bias its inputs:
 *   grad_packed [cubemap_frames,6,N,C]: g_c * w1 * w2 * (1 - f) at the four resolved taps of k0 and g_c * w1 * w2 * f
 *     at those of k1 (f == 0: the taps of k0 alone, weight 1); a corner tap's term times third to each of its three
 *     source texels.  Zero-filled on `stream` by the call (an asynchronous memset, capturable), summed with float
 *     atomics (last bits may differ between calls).
 *   grad_directions [B,H,W,3]: per level dirt_texture_sample_bwd's grad_uv formula with T_k on the resolved tap
 *     values (the corner tap's value is its mean; the fold, the face choice and floor have derivative 0; pass always
 *     holds), gu = gu(k0) * (1 - f) + gu(k1) * f (f == 0: gu(k0)), then dirt_texture_sample_cube_bwd's lines.
 *   grad_lod [B,H,W] (needs lod_in): pass ? sum_c g_c * (s_k1,c - s_k0,c) : 0, pass: lod_in is not NaN and
 *     0 <= lod_in + lod_bias <= L-1.  At an integer lod this is the derivative to the right: level k1 is read although
 *     the forward did not read it.  k1 == k0 gives 0.  The automatic lod carries no gradient.
 *   grad_directions and grad_lod are gathers in a fixed order, bit-identical from run to run, zero at unsampled
 *   pixels.  Each of the three may be NULL; with all NULL, or B == 0, no launch is made.
 * Every argument error is a return code raised before any GPU call. */
int dirt_texture_sample_cube_mip_fwd(const float *packed, int cubemap_frames, int S, int C, int levels,
                                     const float *directions, const uint8_t *mask, const float *lod_in, float lod_bias,
                                     int B, int H, int W, int seamless, float *texels, uint8_t *valid, float *lod,
                                     void *stream);
int dirt_texture_sample_cube_mip_bwd(const float *packed, int cubemap_frames, int S, int C, int levels,
                                     const float *directions, const uint8_t *mask, const float *lod_in, float lod_bias,
                                     const float *lod, int B, int H, int W, int seamless, const float *grad_texels,
                                     float *grad_packed, float *grad_directions, float *grad_lod, void *stream);

/* Shadow-map lookup: the visibility of a light at a world-position G-buffer, and its gradients.
 * depth_map [map_frames,Sh,Sw] (map_frames = 1: shared by the B frames, = B: one per frame) holds the light's
 * clip-space z before the divide, +inf where nothing was drawn; positions [B,H,W,3]; mask [B,H,W] uint8 (NULL = "the
 * three position channels are finite"); light_matrix [4][4], or [B][4][4] with matrix_per_frame, row vectors
 * (clip = [p,1] @ M); bias, softness finite and >= 0, in clip-z units; visibility [B,H,W]; valid [B,H,W] uint8 (0 / 1).
 * H, W, Sh, Sw in 1..DIRT_MAX_DIM, B >= 0 (B == 0: no-op).  Rule, float32, every step one IEEE operation:
 *   c_j = ((p0 * M[0][j] + p1 * M[1][j]) + p2 * M[2][j]) + M[3][j]  (cx, cy, cz, cw);  iw = 1 / cw
 *   u = (cx * iw) * 0.5 + 0.5;  v = 0.5 - (cy * iw) * 0.5;  inside = cw > 0 && 0 <= u <= 1 && 0 <= v <= 1
 * A sampled pixel that is not inside is lit (visibility 1, no gradient, no address); an inside one takes the taps and
 * weights of dirt_texture_sample_*'s DIRT_TEXTURE_CLAMP rule on v with Sh and u with Sw, and per tap with texel d and
 * zc = cz - bias:   softness == 0: s = d >= zc ? 1 : 0
 *                   softness  > 0: t = (d - zc) * (1 / softness) + 1;  s = t < 0 ? 0 : (t > 1 ? 1 : t)
 *   visibility = (s00 * (1 - a) + s01 * a) * (1 - b) + (s10 * (1 - a) + s11 * a) * b
 * Pixels that are not sampled give exactly 0 and valid 0.  Backward, g = grad_visibility[p] at inside pixels (the
 * float32 order is in dirt_amd/csrc/shadow_kernels.h):
 *   grad_depth_map[tap] += g * w_tap * (1 / softness) where softness > 0, d is finite and 0 <= t <= 1: zero-filled
 *     on `stream` by the call (an asynchronous memset, capturable), summed with float atomics (the last bits may
 *     differ between calls); with map_frames = 1 it sums over the frames;
 *   grad_positions [B,H,W,3] = g_c @ M[:3]^T with g_c the adjoint of the clip coordinates (through the ramp into cz,
 *     through u and v into cx, cy and cw): fully overwritten, exactly 0 elsewhere, bit-identical from run to run;
 *   grad_light_matrix [4][4] or [B][4][4]: M[r][j] receives the sum over the pixels of p_r * g_c[j], M[3][j] of
 *     g_c[j] (a shared matrix over all frames in frame order).  It needs `workspace` of
 *     dirt_shadow_sample_workspace() bytes (no clearing): the backward writes one row of 16 partial sums per 16 x 16
 *     screen tile with plain stores and a second launch adds them in a fixed order -- bit-identical from run to run.
 * Each of the three may be NULL; with all NULL, or B == 0, no launch is made.  Every argument error is a return code
 * raised before any GPU call. */
int dirt_shadow_sample_workspace(int B, int H, int W, size_t *bytes);
int dirt_shadow_sample_fwd(const float *depth_map, int map_frames, int Sh, int Sw, const float *positions,
                           const uint8_t *mask, int B, int H, int W, int matrix_per_frame, const float *light_matrix,
                           float bias, float softness, float *visibility, uint8_t *valid, void *stream);
int dirt_shadow_sample_bwd(const float *depth_map, int map_frames, int Sh, int Sw, const float *positions,
                           const uint8_t *mask, int B, int H, int W, int matrix_per_frame, const float *light_matrix,
                           float bias, float softness, const float *grad_visibility, float *grad_depth_map,
                           float *grad_positions, float *grad_light_matrix, void *workspace, size_t workspace_bytes,
                           void *stream);

/* Thread-local message for the last non-OK return on this thread. */
const char *dirt_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* DIRT_MI355X_H */
