"""The pixel-space stage of deferred shading: silhouette dilation and G-buffer lighting.

The reference's sample (samples/deferred.py:85-115) dilates the position and normal G-buffers by a 3x3 max where the
background shows, then adds ambient, diffuse_directional and specular_directional per pixel.  Its blend
`x * (1 - mask) + dilated * mask` turns every background pixel into NaN (-inf * 0); here the blend is a select, pixels
the dilation does not reach are left out of the shading (exactly 0, `valid` False) and no NaN reaches a gradient.

  dilate(x, mask=None)     [H,W,C] or [B,H,W,C]: the 3x3 max where mask is set (default: any channel is +-inf)
  shade(positions, colors, normals, ...) -> (pixels, valid)
  shade_lights(positions, colors, normals, light_vectors, diffuse_colors, specular_colors, camera_position, shininess,
               ambient_color=None, point=None, double_sided=False) -> (pixels, valid): shade under up to 8 directional
                           or point lights, with gradients to the lights, the camera, the ambient colour, the shininess
  shade_pbr(positions, colors, normals, material, light_vectors, light_colors, camera_position, ambient_color=None,
            point=None, visibility=None) -> (pixels, valid): the metallic-roughness model (Lambert + GGX) under up to
                           8 lights with a per-pixel, per-light visibility, with gradients to every input
  shade_sh(colors, normals, coefficients, mask=None, normalize=False) -> (pixels, valid): the colours under 1, 4 or 9
                           spherical-harmonic coefficients of the dilated normals, with gradients to all three
  reflect_view(positions, normals, camera_position) -> (directions, valid): the view vector reflected about the
                           normal, the direction a specular environment is looked up by; (0, 0, 0) where not valid
  shade_env(positions, colors, normals, material, coefficients, radiance, camera_position, occlusion=None) ->
                           (pixels, valid): split-sum image-based lighting of the metallic-roughness material, a
                           spherical-harmonic irradiance plus a prefiltered radiance times the environment BRDF
  sample_texture(texture, uv, mask=None, wrap="clamp") -> (texels, valid): bilinear texture lookup at a uv G-buffer
  build_mipmaps(texture, levels=None) -> Mipmaps: the box-filtered mip chain, packed
  sample_texture_mip(mipmaps_or_texture, uv, mask=None, wrap="clamp", lod=None, lod_bias=0.0) -> (texels, valid):
                           trilinear lookup of the chain, the level chosen per pixel from the uv differences
  sample_cubemap(cubemap, directions, mask=None) -> (texels, valid): bilinear cube-map lookup at a direction G-buffer
  build_cubemap_mipmaps(cubemap, levels=None) -> CubeMipmaps: every face's box-filtered mip chain, packed
  sample_cubemap_mip(chain_or_cubemap, directions, mask=None, lod=None, lod_bias=0.0, seamless=True) -> (texels,
                           valid): trilinear cube-map lookup filtered across the face seams, the level chosen per pixel
                           or given (a roughness map), with a gradient to a given lod
  sample_shadow(depth_map, positions, light_matrix, bias=0.0, softness=0.0, mask=None) -> (visibility, valid): a
                           light's shadow map looked up at the world-position G-buffer, 2 x 2 percentage-closer taps
                           over a soft ramp, with gradients to the map, the positions and the light's matrix

On the GPU both run as one fused HIP launch forward and one backward (dirt_amd/csrc/deferred_kernels.h, C ABI
dirt_dilate_* / dirt_deferred_shade_*) when their operands are float32 tensors on one GPU and the light parameters
are [3] float32 tensors on it that need no gradient, with a Python-number shininess.  Anything else -- CPU tensors,
other dtypes, gradients with respect to the light, a tensor-valued shininess -- runs the framework-op statement below
(`_dilate_ops`, `_shade_ops`).  The max follows the framework's CPU max_pool2d: the first maximum wins ties, a NaN in
the window gives NaN.  The fused backwards are gathers in a fixed order: their gradients are bit-identical from run
to run.  They are kernels, not differentiable graphs: `create_graph=True` through them raises RuntimeError;
DIRT_FUSED_DEFERRED=0 routes every call to the framework ops (double backward supported).

shade_lights is the shade for an inverse renderer that fits the lighting, a camera pose or a material exponent
(dirt_amd/csrc/shade_lights_kernels.h, C ABI dirt_deferred_shade_lights_*; the statement is `_shade_lights_ops`): N
lights in one pass over the G-buffers, and parameters that need a gradient stay on the fused path.  Its backward is two
launches: per-chunk partial sums of the per-pixel parameter terms, then their sum in a fixed order -- no float atomics,
every gradient bit-identical from run to run.  `shade` itself is unchanged.

shade_pbr is the material model the other ops feed (dirt_amd/csrc/shade_pbr_kernels.h, C ABI dirt_deferred_shade_pbr_*;
the statement is `_shade_pbr_ops`): a roughness / metallic map fetched by sample_texture, one visibility per shadowed
light from sample_shadow, N lights in one pass.  Lambert plus a GGX lobe (t = |n x h|^2 + (n.h alpha)^2, the form that
does not cancel in float32), Schlick-GGX visibility and Schlick's Fresnel term, the roughness clamped at 0.045.  One
launch forward, two backward as shade_lights', every gradient -- G-buffers, material, visibility, lights, camera,
ambient colour -- bit-identical from run to run; the same eligibility and fallback.

shade_sh lights the colours with an environment instead: 9 (or 4, or 1) RGB spherical-harmonic coefficients, smooth
in the normal and linear in the unknowns (dirt_amd/csrc/shade_sh_kernels.h, C ABI dirt_deferred_shade_sh_*; the
statement is `_shade_sh_ops`).  One launch forward, two backward as shade_lights', the coefficients' gradient summed in
a fixed order; it needs no positions, and its normals dilate under their own background or an explicit mask.

reflect_view and shade_env join shade_sh, sample_cubemap_mip and shade_pbr into image-based lighting
(dirt_amd/csrc/shade_env_kernels.h, C ABI dirt_deferred_reflect_view_* / dirt_deferred_shade_env_*; the statements are
`_reflect_view_ops`, `_shade_env_ops`):

    directions, _ = reflect_view(positions, normals, camera)
    radiance, _   = sample_cubemap_mip(chain, directions, lod=material[..., 0] * (len(chain) - 1))
    pixels, valid = shade_env(positions, colors, normals, material, coefficients, radiance, camera, occlusion=ao)

Both dilate positions and normals by the shade's rule, so that the silhouette ring agrees with `valid`; a pixel that is
not valid gets the direction (0, 0, 0), which the cube-map lookups leave out.  shade_env uses shade_sh's basis for the
diffuse half and the analytic fit of the split-sum environment BRDF for the specular half.  One launch forward, two
backward as shade_lights', every gradient -- G-buffers, material, radiance, occlusion, coefficients, camera --
bit-identical from run to run; shade_pbr's eligibility and fallback.

sample_texture is the step between the two: UV -> texel, with gradients to the texture and through the uv into the
geometry (dirt_amd/csrc/texture_kernels.h, C ABI dirt_texture_sample_*; the statement is `_sample_texture_ops`).  Its
uv gradient is a gather in a fixed order too; its texture gradient is a scatter-add summed with float atomics (per
screen tile in an LDS patch first), so it may differ in the last bits from run to run, as vertex_normals' does.

build_mipmaps and sample_texture_mip are its minification-safe form (dirt_amd/csrc/texture_mip_kernels.h, C ABI
dirt_texture_mip_* / dirt_texture_sample_mip_*; the statements are `_build_mipmaps_ops`, `_sample_texture_mip_ops`),
with the same eligibility and fallback.  The level of detail is a constant of the backward: it carries no gradient.

sample_cubemap looks a pixel up by direction: the specular half of an environment (a reflection vector) or a sky (the
view ray), with gradients to the cube map's texels and through the direction into the geometry
(dirt_amd/csrc/cubemap_kernels.h, C ABI dirt_texture_sample_cube_*; the statement is `_sample_cubemap_ops`).  A face is
filtered as sample_texture filters a clamped texture, never across a seam; the gradients behave as sample_texture's.

build_cubemap_mipmaps and sample_cubemap_mip are the glossy step between shade_sh and sample_cubemap: the environment
read at a level of detail that grows with the roughness (dirt_amd/csrc/cubemap_mip_kernels.h, C ABI
dirt_texture_sample_cube_mip_*, the chain through dirt_texture_mip_build_* with six faces per frame; the statement is
`_sample_cubemap_mip_ops`).  Every level is filtered across the face seams and the cube's corners, so that an 8 x 8 or
1 x 1 level is no cube with hard edges.  An explicit lod receives a gradient (the difference of its two levels, at an
integer lod the one to the right); the automatic lod, taken from the point on the unit cube, carries none.

sample_shadow lets a light of shade_lights be blocked (dirt_amd/csrc/shadow_kernels.h, C ABI dirt_shadow_sample_*; the
statement is `_sample_shadow_ops`).  The light's depth map is a 1-channel `rasterise` of its clip-space z over +inf;
the lookup projects each pixel's world position with the light's matrix, compares the four bilinear taps with its
clip z over a ramp of width `softness`, and returns the blend: a visibility that multiplies one shade_lights call per
shadowed light.  One launch forward; backward one launch, a workgroup per 16 x 16 screen tile -- the positions'
gradient a gather, the depth map's a scatter-add through sample_texture's LDS patch -- and, when the matrix needs a
gradient (it stays on the fused path), shade_lights' second launch that sums the tiles' partial sums in a fixed order.
"""
import ctypes
import os
import struct

import torch
import torch.nn.functional as Fn

from . import _lib
from .lighting import (_diffuse_directional_ops, _diffuse_point_ops, _gpu_f32, _light_param,
                       _specular_directional_ops)

__all__ = ["dilate", "shade"]

_FUSED_ENABLED = os.environ.get("DIRT_FUSED_DEFERRED", "1") != "0"


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _no_double_backward(fn):
    if torch.is_grad_enabled():
        raise RuntimeError("%s: the fused HIP backward does not support create_graph=True (double backward); "
                           "set DIRT_FUSED_DEFERRED=0 to use the framework-op statement" % fn)


def _batched(x, dim=4):
    """x contiguous with `dim` dimensions, a leading one added where it has one fewer, and whether it was added."""
    x = x.contiguous()
    return (x, False) if x.dim() == dim else (x[None], True)


def _unbatched(results, added):
    """a result or a tuple of results, without the batch dimension that `_batched` added"""
    if not added:
        return results
    return results[0] if isinstance(results, torch.Tensor) else tuple(r[0] for r in results)


def _checked_mask(fn, mask, like, name):
    """mask (or None) as a tensor on like's device, of like's shape without the channels"""
    if mask is not None:
        mask = torch.as_tensor(mask, device=like.device)
        if mask.shape != like.shape[:-1]:
            raise ValueError("%s: mask of shape %s for %s of shape %s"
                             % (fn, tuple(mask.shape), name, tuple(like.shape)))
    return mask


def _kernel_mask(mask, batched):
    """mask (or None) as the kernels read it: uint8 0 / 1 over the pixels of the batched operand"""
    if mask is None:
        return None
    return (mask if mask.dtype == torch.bool else mask != 0).contiguous().view(torch.uint8).reshape(batched.shape[:-1])


def _gbuffers(fn, positions, colors, normals):
    """the three G-buffers as tensors of positions' dtype and device, their shapes checked"""
    positions = torch.as_tensor(positions)
    colors, normals = (torch.as_tensor(x, dtype=positions.dtype, device=positions.device) for x in (colors, normals))
    if positions.dim() not in (3, 4) or positions.shape[-1] != 3 or colors.shape != positions.shape or \
            normals.shape != positions.shape:
        raise ValueError("%s: positions, colors, normals must share one shape [H, W, 3] or [B, H, W, 3]" % fn)
    return positions, colors, normals


# ---- dilation

def _dilate_ops(x, mask=None):
    """x [H,W,C] or [B,H,W,C]; mask (x's shape without the channels) or None."""
    m = torch.isinf(x).any(-1, keepdim=True) if mask is None else (mask != 0)[..., None]
    if x.dim() == 3:
        pooled = Fn.max_pool2d(x.permute(2, 0, 1)[None], 3, stride=1, padding=1)[0].permute(1, 2, 0)
    else:
        pooled = Fn.max_pool2d(x.permute(0, 3, 1, 2), 3, stride=1, padding=1).permute(0, 2, 3, 1)
    return torch.where(m, pooled, x)


class _DilateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        B, H, W, C = x.shape
        out = torch.empty_like(x)
        route = torch.empty((B, H, W), dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dirt_dilate_fwd(x.data_ptr(), _ptr(mask), B, H, W, C, out.data_ptr(),
                                                   route.data_ptr(), _stream(x.device)))
        ctx.save_for_backward(route)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        _no_double_backward("dilate")
        route, = ctx.saved_tensors
        B, H, W = route.shape
        grad_out = grad_out.contiguous()
        grad_x = torch.empty_like(grad_out)
        with torch.cuda.device(route.device):
            _lib.check(_lib.load().dirt_dilate_bwd(grad_out.data_ptr(), route.data_ptr(), B, H, W, grad_out.shape[-1],
                                                   grad_x.data_ptr(), _stream(route.device)))
        return grad_x, None


def dilate(x, mask=None):
    """The 3x3 max of x ([H,W,C] or [B,H,W,C]) where mask ([H,W] or [B,H,W], nonzero = dilate) is set, x elsewhere;
    mask=None dilates the pixels with a channel at +inf or -inf (a G-buffer's background)."""
    x = torch.as_tensor(x)
    if x.dim() not in (3, 4):
        raise ValueError("dilate: x must be [H, W, C] or [B, H, W, C]")
    mask = _checked_mask("dilate", mask, x, "x")
    if (_FUSED_ENABLED and _gpu_f32(x) and 1 <= x.shape[-1] <= _lib.MAX_CHANNELS and
            (mask is None or mask.device == x.device)):
        xb, added = _batched(x)
        return _unbatched(_DilateFn.apply(xb, _kernel_mask(mask, xb)), added)
    return _dilate_ops(x, mask)


# ---- shade

def _dilated_gbuffers(positions, colors, normals):
    """The statement's opening: positions and normals dilated under the positions' background, `valid` where both are
    finite, and the three G-buffers zero-filled elsewhere -> (positions, normals, colors, valid)."""
    bg = torch.isinf(positions).any(-1)
    pos_d = _dilate_ops(positions, bg)
    nrm_d = _dilate_ops(normals, bg)
    valid = torch.isfinite(pos_d).all(-1, keepdim=True) & torch.isfinite(nrm_d).all(-1, keepdim=True)
    return tuple(torch.where(valid, x, 0.0) for x in (pos_d, nrm_d, colors)) + (valid,)


def _shade_ops(positions, colors, normals, ambient_color, light_direction, diffuse_color, specular_color,
               camera_position, shininess, double_sided=False):
    dev, dt = positions.device, positions.dtype
    pos_s, nrm_s, col_s, valid = _dilated_gbuffers(positions, colors, normals)
    ambient = col_s * torch.as_tensor(ambient_color, dtype=dt, device=dev)
    diffuse = _diffuse_directional_ops(nrm_s.reshape(-1, 3), col_s.reshape(-1, 3), light_direction, diffuse_color,
                                       double_sided)
    specular = _specular_directional_ops(pos_s.reshape(-1, 3), nrm_s.reshape(-1, 3), col_s.reshape(-1, 3),
                                         light_direction, specular_color, camera_position, shininess, double_sided)
    pixels = diffuse.reshape(positions.shape) + specular.reshape(positions.shape) + ambient
    return pixels, valid


class _ShadeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, colors, normals, ambient, ldir, dcol, scol, cam, shininess, double_sided):
        B, H, W, _ = positions.shape
        dev = positions.device
        pixels = torch.empty_like(positions)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        route = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_deferred_shade_fwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), B, H, W, ambient.data_ptr(),
                ldir.data_ptr(), dcol.data_ptr(), scol.data_ptr(), cam.data_ptr(), shininess, double_sided,
                pixels.data_ptr(), valid.data_ptr(), route.data_ptr(), _stream(dev)))
        ctx.save_for_backward(positions, colors, normals, ambient, ldir, dcol, scol, cam, route)
        ctx.shininess, ctx.double_sided = shininess, double_sided
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # (no zero-filled "gradient" of valid: one launch less per backward)
        return pixels, valid

    @staticmethod
    def backward(ctx, grad_pixels, _grad_valid):
        _no_double_backward("shade")
        if grad_pixels is None:
            return (None,) * 10
        positions, colors, normals, ambient, ldir, dcol, scol, cam, route = ctx.saved_tensors
        B, H, W, _ = positions.shape
        dev = positions.device
        grad_pixels = grad_pixels.contiguous()
        # (NULL for the gradients nobody needs: the kernel then skips them)
        grads = [torch.empty_like(positions) if need else None for need in ctx.needs_input_grad[:3]]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_deferred_shade_bwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), B, H, W, ambient.data_ptr(),
                ldir.data_ptr(), dcol.data_ptr(), scol.data_ptr(), cam.data_ptr(), ctx.shininess, ctx.double_sided,
                grad_pixels.data_ptr(), route.data_ptr(), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]),
                _stream(dev)))
        return grads[0], grads[1], grads[2], None, None, None, None, None, None, None


def shade(positions, colors, normals, ambient_color, light_direction, diffuse_color, specular_color, camera_position,
          shininess, double_sided=False):
    """Deferred shading of the G-buffers positions, colors, normals ([H,W,3] or [B,H,W,3]; positions and normals over
    a -inf background): positions and normals dilated where the positions' background shows, then
    pixels = diffuse_directional + specular_directional + colors * ambient_color under one directional light
    (diffuse_color and specular_color are its two colours, the colours serve as reflectivities).

    Returns (pixels, valid): valid [..., H, W, 1] bool marks the pixels whose dilated position and normal are finite;
    the others shade to exactly 0 and carry no gradient."""
    positions, colors, normals = _gbuffers("shade", positions, colors, normals)
    if _FUSED_ENABLED and _gpu_f32(positions, colors, normals) and isinstance(shininess, (int, float)):
        ps = [_light_param(x, positions) for x in (ambient_color, light_direction, diffuse_color, specular_color,
                                                   camera_position)]
        if all(p is not None for p in ps):
            ops, added = zip(*(_batched(x) for x in (positions, colors, normals)))
            return _unbatched(_ShadeFn.apply(*ops, *ps, float(shininess), 1 if double_sided else 0), added[0])
    return _shade_ops(positions, colors, normals, ambient_color, light_direction, diffuse_color, specular_color,
                      camera_position, shininess, double_sided)


# ---- shade_lights: many lights, with gradients to them

def _specular_point_ops(positions, normals, reflectivities, light_position, light_color, camera_position, shininess,
                        double_sided):
    """`_specular_directional_ops` with the unit vector from the light's position to each point in place of the light
    direction (`_diffuse_point_ops`' incident vector): operands [*, V, 3], light parameters [*, 3]."""
    rel = positions - light_position[..., None, :]
    incident = rel / (torch.linalg.norm(rel, dim=-1, keepdim=True) + 1.e-12)
    reflected = incident + 2. * (normals * -incident).sum(-1, keepdim=True) * normals
    to_camera = camera_position[..., None, :] - positions
    cosines = ((to_camera / torch.linalg.norm(to_camera, dim=-1, keepdim=True) + 1.e-12) * reflected).sum(-1, keepdim=True)
    cosines = cosines.abs() if double_sided else cosines.clamp_min(0.)
    return light_color[..., None, :] * reflectivities * torch.pow(cosines, shininess)


def _shade_lights_ops(positions, colors, normals, light_vectors, diffuse_colors, specular_colors, camera_position,
                      shininess, ambient_color=None, point=None, double_sided=False):
    """The framework-op statement of shade_lights: light arrays [N,3] or [B,N,3], camera [3] or [B,3]."""
    dev, dt = positions.device, positions.dtype
    as_t = lambda x: torch.as_tensor(x, dtype=dt, device=dev)  # noqa: E731
    *buffers, valid = _dilated_gbuffers(positions, colors, normals)
    frames = positions.shape[0] if positions.dim() == 4 else 1
    pos_s, nrm_s, col_s = (x.reshape(frames, -1, 3) for x in buffers)
    vectors, diffuse, specular, camera = (as_t(x) for x in (light_vectors, diffuse_colors, specular_colors,
                                                            camera_position))
    if isinstance(shininess, torch.Tensor):
        shininess = as_t(shininess).reshape(())
    # (the ambient term first, as `_shade_ops` forms it: autograd then adds the colour's three gradients in its order)
    ambient = None if ambient_color is None else col_s * as_t(ambient_color)

    def lit(pos, nrm, col, vectors, diffuse, specular, camera):
        """the lights' sum over rows [R,3] under one set of lights [N,3] and one camera [3]"""
        acc = None
        for i in range(vectors.shape[0]):
            if point is not None and point[i]:
                d = _diffuse_point_ops(pos, nrm, col, vectors[i], diffuse[i], double_sided)
                s = _specular_point_ops(pos, nrm, col, vectors[i], specular[i], camera, shininess, double_sided)
            else:
                d = _diffuse_directional_ops(nrm, col, vectors[i], diffuse[i], double_sided)
                s = _specular_directional_ops(pos, nrm, col, vectors[i], specular[i], camera, shininess, double_sided)
            acc = d + s if acc is None else acc + (d + s)
        return torch.zeros_like(col) if acc is None else acc

    if vectors.dim() == 3 or camera.dim() == 2:
        per = lambda x, d, b: x[b] if x.dim() == d else x  # noqa: E731
        acc = torch.stack([lit(pos_s[b], nrm_s[b], col_s[b], per(vectors, 3, b), per(diffuse, 3, b),
                               per(specular, 3, b), per(camera, 2, b)) for b in range(frames)])
    else:
        acc = lit(pos_s.reshape(-1, 3), nrm_s.reshape(-1, 3), col_s.reshape(-1, 3), vectors, diffuse, specular,
                  camera).reshape(col_s.shape)
    if ambient is not None:
        acc = acc + ambient
    return acc.reshape(positions.shape), valid


def _point_mask(point):
    return sum(1 << i for i, on in enumerate(point or ()) if on)


class _ShadeLightsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, colors, normals, vectors, diffuse, specular, camera, ambient, shininess_t,
                shininess, mask, double_sided):
        B, H, W, _ = positions.shape
        dev = positions.device
        pixels = torch.empty_like(positions)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        route = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        ctx.args = (vectors.shape[-2], mask, 1 if vectors.dim() == 3 else 0, 1 if camera.dim() == 2 else 0,
                    shininess, double_sided)
        n, mask, lights_pf, cam_pf, shininess, double_sided = ctx.args
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_deferred_shade_lights_fwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), B, H, W, _ptr(ambient), n, mask,
                lights_pf, vectors.data_ptr(), diffuse.data_ptr(), specular.data_ptr(), cam_pf, camera.data_ptr(),
                shininess, _ptr(shininess_t), double_sided, pixels.data_ptr(), valid.data_ptr(), route.data_ptr(),
                _stream(dev)))
        ctx.save_for_backward(positions, colors, normals, vectors, diffuse, specular, camera, ambient, shininess_t,
                              route)
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # (as the shade: no zero-filled "gradient" of valid)
        return pixels, valid

    @staticmethod
    def backward(ctx, grad_pixels, _grad_valid):
        _no_double_backward("shade_lights")
        if grad_pixels is None:
            return (None,) * 12
        positions, colors, normals, vectors, diffuse, specular, camera, ambient, shininess_t, route = ctx.saved_tensors
        n, mask, lights_pf, cam_pf, shininess, double_sided = ctx.args
        B, H, W, _ = positions.shape
        dev = positions.device
        grad_pixels = grad_pixels.contiguous()
        # (NULL for the gradients nobody needs: the kernels then skip them, and with no parameter among them the
        # partial sums and the second launch as well)
        saved = (positions, colors, normals, vectors, diffuse, specular, camera, ambient, shininess_t)
        grads = [torch.empty_like(t) if need and t is not None else None
                 for t, need in zip(saved, ctx.needs_input_grad[:9])]
        lib = _lib.load()
        workspace, size = None, _lib._SZ(0)
        if any(g is not None for g in grads[3:]):
            _lib.check(lib.dirt_deferred_shade_lights_workspace(B, H, W, n, ctypes.byref(size)))
            workspace = torch.empty((max(size.value, 4),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.dirt_deferred_shade_lights_bwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), B, H, W, _ptr(ambient), n, mask,
                lights_pf, vectors.data_ptr(), diffuse.data_ptr(), specular.data_ptr(), cam_pf, camera.data_ptr(),
                shininess, _ptr(shininess_t), double_sided, grad_pixels.data_ptr(), route.data_ptr(),
                _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[7]), _ptr(grads[3]), _ptr(grads[4]),
                _ptr(grads[5]), _ptr(grads[6]), _ptr(grads[8]), _ptr(workspace), size.value, _stream(dev)))
        return tuple(grads) + (None, None, None)


def _lights_param(x, like, shapes):
    """A light parameter usable by the fused kernels (a float32 tensor on like's device of one of `shapes`; it may
    need a gradient), else None."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != like.device or \
            tuple(x.shape) not in shapes:
        return None
    return x.contiguous()


def shade_lights(positions, colors, normals, light_vectors, diffuse_colors, specular_colors, camera_position,
                 shininess, ambient_color=None, point=None, double_sided=False):
    """`shade` under N lights (0 <= N <= 8; N = 0 is ambient only), with gradients to the lights.

    positions, colors, normals: the G-buffers, as for `shade`.  light_vectors, diffuse_colors, specular_colors: [N,3]
    shared by the frames or [B,N,3] one set per frame, all three in the same form.  point: None (all directional) or
    N Python bools; a directional light's row of light_vectors is its direction (used raw, as diffuse_directional
    does), a point light's row is its position.  camera_position: [3] or [B,3].  shininess: a Python number, or a
    one-element tensor (which can receive a gradient).  ambient_color: [3], or None for zero.

    For a valid pixel, lights in index order: acc = (d_0 + s_0), acc = acc + (d_i + s_i), pixels = acc + colors *
    ambient_color, with d_i, s_i = diffuse_directional, specular_directional for a directional light, and for a point
    light diffuse_point and specular_directional with u = (p - light) / (|p - light| + 1e-12) as its direction (no
    distance attenuation).  Dilation and (pixels, valid) are `shade`'s.

    On the GPU (float32 tensors on one device) the forward is one fused launch and the backward two, whichever inputs
    need gradients: the G-buffers, the light arrays, the camera, the ambient colour and a tensor shininess.  A
    parameter's gradient is the sum of its per-pixel terms in a fixed order: bit-identical from run to run."""
    fn = "shade_lights"
    positions, colors, normals = _gbuffers(fn, positions, colors, normals)
    dev, dt = positions.device, positions.dtype
    lights = [x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=dt, device=dev)
              for x in (light_vectors, diffuse_colors, specular_colors)]
    if any(x.dim() not in (2, 3) or x.shape[-1] != 3 for x in lights):
        raise ValueError("%s: light_vectors, diffuse_colors, specular_colors must be [N, 3] or [B, N, 3]" % fn)
    if len({x.dim() for x in lights}) != 1:
        raise ValueError("%s: the three light arrays must all be shared [N, 3] or all per frame [B, N, 3]" % fn)
    if len({x.shape[-2] for x in lights}) != 1:
        raise ValueError("%s: the three light arrays hold %s lights" % (fn, [x.shape[-2] for x in lights]))
    n = lights[0].shape[-2]
    if n > _lib.MAX_LIGHTS:
        raise ValueError("%s: %d lights, at most %d" % (fn, n, _lib.MAX_LIGHTS))
    frames = positions.shape[0] if positions.dim() == 4 else None
    if lights[0].dim() == 3 and any(x.shape[0] != frames for x in lights):
        raise ValueError("%s: per-frame light arrays need one set per frame of a [B, H, W, 3] batch" % fn)
    if point is not None:
        point = tuple(bool(b) for b in point)
        if len(point) != n:
            raise ValueError("%s: point has %d entries for %d lights" % (fn, len(point), n))
    if not isinstance(camera_position, torch.Tensor):
        camera_position = torch.as_tensor(camera_position, dtype=dt, device=dev)
    if tuple(camera_position.shape) not in ((3,), (frames, 3)):
        raise ValueError("%s: camera_position must be [3] or [B, 3]" % fn)
    if isinstance(shininess, torch.Tensor) and shininess.numel() != 1:
        raise ValueError("%s: shininess must be a number or a one-element tensor" % fn)
    if _FUSED_ENABLED and _gpu_f32(positions, colors, normals) and \
            (isinstance(shininess, (int, float)) or _gpu_f32(positions, shininess)):
        light_shape = ((n, 3),) if lights[0].dim() == 2 else ((frames, n, 3),)
        ps = [_lights_param(x, positions, light_shape) for x in lights]
        ps.append(_lights_param(camera_position, positions, ((3,), (frames, 3))))
        amb = None if ambient_color is None else _lights_param(ambient_color, positions, ((3,),))
        if all(p is not None for p in ps) and (ambient_color is None or amb is not None):
            ops, added = zip(*(_batched(x) for x in (positions, colors, normals)))
            number = isinstance(shininess, (int, float))
            return _unbatched(_ShadeLightsFn.apply(*ops, *ps, amb, None if number else shininess.contiguous(),
                                                   float(shininess) if number else 0.0, _point_mask(point),
                                                   1 if double_sided else 0), added[0])
    return _shade_lights_ops(positions, colors, normals, lights[0], lights[1], lights[2], camera_position, shininess,
                             ambient_color, point, double_sided)


# ---- shade_pbr: metallic-roughness GGX lighting

def _shade_pbr_ops(positions, colors, normals, material, light_vectors, light_colors, camera_position,
                   ambient_color=None, point=None, visibility=None):
    """The framework-op statement of shade_pbr, each line one operation: G-buffers [H,W,3] or [B,H,W,3], material
    [...,2], light arrays [N,3] or [B,N,3], camera [3] or [B,3], visibility [...,N] or None (ones)."""
    dev, dt = positions.device, positions.dtype
    as_t = lambda x: torch.as_tensor(x, dtype=dt, device=dev)  # noqa: E731
    *buffers, valid = _dilated_gbuffers(positions, colors, normals)
    frames = positions.shape[0] if positions.dim() == 4 else 1
    pos_s, nrm_s, col_s = (x.reshape(frames, -1, 3) for x in buffers)
    mat_s = torch.where(valid, as_t(material), 0.0).reshape(frames, -1, 2)
    vectors, lcolors, camera = (as_t(x) for x in (light_vectors, light_colors, camera_position))
    n_lights = vectors.shape[-2]
    vis_s = None
    if visibility is not None and n_lights:
        vis_s = torch.where(valid, as_t(visibility), 0.0).reshape(frames, -1, n_lights)
    ambient = None if ambient_color is None else col_s * as_t(ambient_color)
    r_min, pi = _lib.PBR_MIN_ROUGHNESS, 3.141592653589793

    def unit(x):
        length = torch.linalg.norm(x, dim=-1, keepdim=True)
        length = length + 1.e-12
        return x / length

    def lit(pos, nrm, col, mat, vis, vectors, lcolors, camera):
        """the lights' sum over rows [R,3] under one set of lights [N,3] and one camera [3]"""
        n = unit(nrm)
        to_camera = camera - pos
        v = unit(to_camera)
        r = torch.clamp(mat[:, 0:1], r_min, 1.0)
        m = torch.clamp(mat[:, 1:2], 0.0, 1.0)
        alpha = r * r
        k = alpha * 0.5
        omk = 1.0 - k
        alpha2 = alpha * alpha
        nv = (n * v).sum(-1, keepdim=True)
        nv = nv.clamp_min(0.0)
        gv = nv * omk
        gv = gv + k
        f0 = col - 0.04
        f0 = f0 * m
        f0 = 0.04 + f0
        omf0 = 1.0 - f0
        om = 1.0 - m
        acc = None
        for i in range(n_lights):
            if point is not None and point[i]:
                l = unit(vectors[i] - pos)
            else:
                l = unit(-vectors[i])
            h = unit(l + v)
            nl = (n * l).sum(-1, keepdim=True)
            lit_i = nl > 0
            nls = torch.where(lit_i, nl, 1.0)  # (the unlit side is a select: nothing of it reaches a gradient)
            nh = (n * h).sum(-1, keepdim=True)
            vh = (v * h).sum(-1, keepdim=True)
            vh = torch.clamp(vh, 0.0, 1.0)
            x = torch.linalg.cross(n, h)
            xx = (x * x).sum(-1, keepdim=True)
            a = nh * alpha
            aa = a * a
            t = xx + aa
            has_t = t > 0
            ts = torch.where(has_t, t, 1.0)
            t2 = ts * ts
            t2 = pi * t2
            D = alpha2 / t2
            D = torch.where(has_t, D, 0.0)
            gl = nls * omk
            gl = gl + k
            glgv = gl * gv
            glgv = 4.0 * glgv
            V = 1.0 / glgv
            w = 1.0 - vh
            w2 = w * w
            w4 = w2 * w2
            w5 = w4 * w
            F = omf0 * w5
            F = f0 + F
            dd = 1.0 - F
            dd = dd * om
            dd = dd * col
            dd = dd / pi
            e = lcolors[i] * nls
            DV = D * V
            s = DV * F
            d = e * dd
            s = e * s
            term = d + s
            if vis is not None:
                term = vis[:, i:i + 1] * term
            term = torch.where(lit_i, term, 0.0)
            acc = term if acc is None else acc + term
        return torch.zeros_like(col) if acc is None else acc

    if vectors.dim() == 3 or camera.dim() == 2:
        per = lambda x, d, b: x[b] if x.dim() == d else x  # noqa: E731
        acc = torch.stack([lit(pos_s[b], nrm_s[b], col_s[b], mat_s[b], None if vis_s is None else vis_s[b],
                               per(vectors, 3, b), per(lcolors, 3, b), per(camera, 2, b)) for b in range(frames)])
    else:
        acc = lit(pos_s.reshape(-1, 3), nrm_s.reshape(-1, 3), col_s.reshape(-1, 3), mat_s.reshape(-1, 2),
                  None if vis_s is None else vis_s.reshape(-1, n_lights), vectors, lcolors,
                  camera).reshape(col_s.shape)
    if ambient is not None:
        acc = acc + ambient
    return torch.where(valid, acc.reshape(positions.shape), 0.0), valid


class _ShadePbrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, colors, normals, material, visibility, vectors, lcolors, camera, ambient, mask):
        B, H, W, _ = positions.shape
        dev = positions.device
        pixels = torch.empty_like(positions)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        route = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        ctx.args = (vectors.shape[-2], mask, 1 if vectors.dim() == 3 else 0, 1 if camera.dim() == 2 else 0)
        n, mask, lights_pf, cam_pf = ctx.args
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_deferred_shade_pbr_fwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), material.data_ptr(), _ptr(visibility),
                B, H, W, _ptr(ambient), n, mask, lights_pf, vectors.data_ptr(), lcolors.data_ptr(), cam_pf,
                camera.data_ptr(), pixels.data_ptr(), valid.data_ptr(), route.data_ptr(), _stream(dev)))
        ctx.save_for_backward(positions, colors, normals, material, visibility, vectors, lcolors, camera, ambient,
                              route)
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # (as the shade: no zero-filled "gradient" of valid)
        return pixels, valid

    @staticmethod
    def backward(ctx, grad_pixels, _grad_valid):
        _no_double_backward("shade_pbr")
        if grad_pixels is None:
            return (None,) * 10
        *saved, route = ctx.saved_tensors
        positions, colors, normals, material, visibility, vectors, lcolors, camera, ambient = saved
        n, mask, lights_pf, cam_pf = ctx.args
        B, H, W, _ = positions.shape
        dev = positions.device
        grad_pixels = grad_pixels.contiguous()
        # (NULL for the gradients nobody needs: the kernels then skip them, and with no parameter among them the
        # partial sums and the second launch as well)
        grads = [torch.empty_like(t) if need and t is not None else None
                 for t, need in zip(saved, ctx.needs_input_grad[:9])]
        lib = _lib.load()
        workspace, size = None, _lib._SZ(0)
        if any(g is not None for g in grads[5:]):
            _lib.check(lib.dirt_deferred_shade_pbr_workspace(B, H, W, n, ctypes.byref(size)))
            workspace = torch.empty((max(size.value, 4),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.dirt_deferred_shade_pbr_bwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), material.data_ptr(), _ptr(visibility),
                B, H, W, _ptr(ambient), n, mask, lights_pf, vectors.data_ptr(), lcolors.data_ptr(), cam_pf,
                camera.data_ptr(), grad_pixels.data_ptr(), route.data_ptr(), _ptr(grads[0]), _ptr(grads[1]),
                _ptr(grads[2]), _ptr(grads[3]), _ptr(grads[4]), _ptr(grads[8]), _ptr(grads[5]), _ptr(grads[6]),
                _ptr(grads[7]), _ptr(workspace), size.value, _stream(dev)))
        return tuple(grads) + (None,)


def shade_pbr(positions, colors, normals, material, light_vectors, light_colors, camera_position,
              ambient_color=None, point=None, visibility=None):
    """The glTF-style metallic-roughness model -- Lambert plus a GGX microfacet lobe -- under N lights (0 <= N <= 8;
    N = 0 is ambient only), with a per-pixel, per-light visibility and gradients to everything.

    positions, colors, normals: the G-buffers, as for `shade`; colors is the base colour.  material [...,H,W,2]:
    channel 0 the perceptual roughness, channel 1 the metallic.  light_vectors, light_colors: [N,3] shared by the
    frames or [B,N,3] one set per frame, both in the same form.  point: None (all directional) or N Python bools; a
    directional light's row is its direction of travel, a point light's row its position.  camera_position: [3] or
    [B,3].  ambient_color: [3], or None for zero.  visibility: None (all ones) or [...,H,W,N], one factor per pixel
    and light: a `sample_shadow` result, a distance attenuation, a spot cone, or their product.  It is read at the
    pixel itself, never dilated, as colors and material are: a caller who wants the dilated silhouette ring lit must
    compute it there, e.g. call `sample_shadow` on `dilate(positions)`.

    Dilation of positions and normals, `valid` and the returned (pixels, valid) are `shade`'s.  For a valid pixel
    with dilated position p, dilated normal n_d and colour c, u(x) = x / (|x| + 1e-12) (subgradient 0 at 0):

        n = u(n_d)   v = u(camera - p)   l_i = u(-direction_i) or u(position_i - p)   h_i = u(l_i + v)
        r = clamp(material_0, 0.045, 1)   m = clamp(material_1, 0, 1)   alpha = r^2   k = alpha / 2
        nl = n . l   nv = max(n . v, 0)   nh = n . h   vh = clamp(v . h, 0, 1)
        t = |n x h|^2 + (nh alpha)^2      D = alpha^2 / (pi t^2) where t > 0, else 0
        V = 1 / (4 (nl (1 - k) + k) (nv (1 - k) + k))
        F0 = 0.04 + (c - 0.04) m          F = F0 + (1 - F0) (1 - vh)^5
        d_i = lc_i nl (1 - F) (1 - m) c / pi          s_i = lc_i nl D V F
        term_i = visibility_i (d_i + s_i) where nl > 0, exactly 0 with no gradient elsewhere
        pixels = term_0 + term_1 + ... + c * ambient_color

    A point light has no distance attenuation: that is a visibility factor.  Every clamp takes torch.clamp's
    derivative, so a roughness below 0.045 receives a zero gradient.  With float32 arithmetic the forward error grows
    as the roughness falls: on the GGX peak with roughness in [0, 0.2) the framework ops measured W = 2.32 of the bound
    that roughness >= 0.2 is held to.

    On the GPU (float32 tensors on one device) the forward is one fused launch and the backward two, whichever inputs
    need gradients: the G-buffers, the material, the visibility, the light arrays, the camera and the ambient colour.
    A parameter's gradient is the sum of its per-pixel terms in a fixed order: bit-identical from run to run."""
    fn = "shade_pbr"
    positions, colors, normals = _gbuffers(fn, positions, colors, normals)
    dev, dt = positions.device, positions.dtype
    if not isinstance(material, torch.Tensor):
        material = torch.as_tensor(material, dtype=dt, device=dev)
    if material.shape != positions.shape[:-1] + (2,):
        raise ValueError("%s: material of shape %s for positions of shape %s; it must be [..., H, W, 2]"
                         % (fn, tuple(material.shape), tuple(positions.shape)))
    lights = [x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=dt, device=dev)
              for x in (light_vectors, light_colors)]
    if any(x.dim() not in (2, 3) or x.shape[-1] != 3 for x in lights):
        raise ValueError("%s: light_vectors, light_colors must be [N, 3] or [B, N, 3]" % fn)
    if len({x.dim() for x in lights}) != 1:
        raise ValueError("%s: the two light arrays must both be shared [N, 3] or both per frame [B, N, 3]" % fn)
    if len({x.shape[-2] for x in lights}) != 1:
        raise ValueError("%s: the two light arrays hold %s lights" % (fn, [x.shape[-2] for x in lights]))
    n = lights[0].shape[-2]
    if n > _lib.MAX_LIGHTS:
        raise ValueError("%s: %d lights, at most %d" % (fn, n, _lib.MAX_LIGHTS))
    frames = positions.shape[0] if positions.dim() == 4 else None
    if lights[0].dim() == 3 and any(x.shape[0] != frames for x in lights):
        raise ValueError("%s: per-frame light arrays need one set per frame of a [B, H, W, 3] batch" % fn)
    if point is not None:
        point = tuple(bool(b) for b in point)
        if len(point) != n:
            raise ValueError("%s: point has %d entries for %d lights" % (fn, len(point), n))
    if not isinstance(camera_position, torch.Tensor):
        camera_position = torch.as_tensor(camera_position, dtype=dt, device=dev)
    if tuple(camera_position.shape) not in ((3,), (frames, 3)):
        raise ValueError("%s: camera_position must be [3] or [B, 3]" % fn)
    if visibility is not None:
        if not isinstance(visibility, torch.Tensor):
            visibility = torch.as_tensor(visibility, dtype=dt, device=dev)
        if visibility.shape != positions.shape[:-1] + (n,):
            raise ValueError("%s: visibility of shape %s for %d lights; it must be [..., H, W, %d]"
                             % (fn, tuple(visibility.shape), n, n))
    if _FUSED_ENABLED and _gpu_f32(positions, colors, normals, material) and \
            (visibility is None or _gpu_f32(positions, visibility)):
        light_shape = ((n, 3),) if lights[0].dim() == 2 else ((frames, n, 3),)
        ps = [_lights_param(x, positions, light_shape) for x in lights]
        ps.append(_lights_param(camera_position, positions, ((3,), (frames, 3))))
        amb = None if ambient_color is None else _lights_param(ambient_color, positions, ((3,),))
        if all(p is not None for p in ps) and (ambient_color is None or amb is not None):
            ops, added = zip(*(_batched(x) for x in (positions, colors, normals, material)))
            vis = None if visibility is None or n == 0 else _batched(visibility)[0]
            return _unbatched(_ShadePbrFn.apply(*ops, vis, *ps, amb, _point_mask(point)), added[0])
    return _shade_pbr_ops(positions, colors, normals, material, lights[0], lights[1], camera_position,
                          ambient_color, point, visibility)


# ---- shade_sh: spherical-harmonic lighting

# the basis constants, as float32 rounds them (the kernels' values, whatever the dtype of the statement)
_SH_C = tuple(struct.unpack("f", struct.pack("f", c))[0] for c in (
    0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396))
_SH_COUNTS = (1, 4, 9)


def _sh_irradiance_ops(n, coefficients):
    """E [...,H,W,3] of the vectors n [...,H,W,3] under coefficients [K,3] or [B,K,3]: shade_sh's basis and order of
    additions, each line one operation."""
    c0, c1, c2, c3, c4 = _SH_C
    x, y, z = n[..., 0:1], n[..., 1:2], n[..., 2:3]
    K = coefficients.shape[-2]
    if coefficients.dim() == 3:
        row = lambda k: coefficients[:, k][:, None, None, :]  # noqa: E731
    else:
        row = lambda k: coefficients[k]  # noqa: E731
    Y = [c0]
    if K > 1:
        Y += [c1 * y, c1 * z, c1 * x]
    if K > 4:
        xy = x * y
        yz = y * z
        zz = z * z
        zz3 = 3.0 * zz
        zz31 = zz3 - 1.0
        xz = x * z
        xx = x * x
        yy = y * y
        xxyy = xx - yy
        Y += [c2 * xy, c2 * yz, c3 * zz31, c2 * xz, c4 * xxyy]
    E = row(0) * Y[0]
    for k in range(1, K):
        term = row(k) * Y[k]
        E = E + term
    return E


def _shade_sh_ops(colors, normals, coefficients, mask=None, normalize=False):
    """The framework-op statement of shade_sh, each line one operation: colors, normals [H,W,3] or [B,H,W,3],
    coefficients [K,3] or [B,K,3], mask (the normals' shape without the channels) or None."""
    m = torch.isinf(normals).any(-1) if mask is None else mask != 0
    nrm_d = _dilate_ops(normals, m)
    valid = torch.isfinite(nrm_d).all(-1, keepdim=True)
    n = torch.where(valid, nrm_d, 0.0)
    col = torch.where(valid, colors, 0.0)
    if normalize:
        length = torch.linalg.norm(n, dim=-1, keepdim=True)
        length = length + 1.e-12
        n = n / length
    E = _sh_irradiance_ops(n, coefficients)
    pixels = col * E
    return torch.where(valid, pixels, 0.0), valid


class _ShadeShFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, normals, coefficients, mask, normalize):
        B, H, W, _ = colors.shape
        dev = colors.device
        pixels = torch.empty_like(colors)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        route = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        ctx.args = (coefficients.shape[-2], 1 if coefficients.dim() == 3 else 0, normalize)
        K, per_frame, normalize = ctx.args
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_deferred_shade_sh_fwd(
                colors.data_ptr(), normals.data_ptr(), _ptr(mask), B, H, W, K, per_frame, coefficients.data_ptr(),
                normalize, pixels.data_ptr(), valid.data_ptr(), route.data_ptr(), _stream(dev)))
        ctx.save_for_backward(colors, normals, coefficients, route)
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # (as the shade: no zero-filled "gradient" of valid)
        return pixels, valid

    @staticmethod
    def backward(ctx, grad_pixels, _grad_valid):
        _no_double_backward("shade_sh")
        if grad_pixels is None:
            return (None,) * 5
        colors, normals, coefficients, route = ctx.saved_tensors
        K, per_frame, normalize = ctx.args
        B, H, W, _ = colors.shape
        dev = colors.device
        grad_pixels = grad_pixels.contiguous()
        # (NULL for the gradients nobody needs: the kernels then skip them, and without the coefficients' the partial
        # sums and the second launch as well)
        grads = [torch.empty_like(t) if need else None
                 for t, need in zip((colors, normals, coefficients), ctx.needs_input_grad[:3])]
        lib = _lib.load()
        workspace, size = None, _lib._SZ(0)
        if grads[2] is not None:
            _lib.check(lib.dirt_deferred_shade_sh_workspace(B, H, W, K, ctypes.byref(size)))
            workspace = torch.empty((max(size.value, 4),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.dirt_deferred_shade_sh_bwd(
                colors.data_ptr(), normals.data_ptr(), B, H, W, K, per_frame, coefficients.data_ptr(), normalize,
                grad_pixels.data_ptr(), route.data_ptr(), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]),
                _ptr(workspace), size.value, _stream(dev)))
        return tuple(grads) + (None, None)


def shade_sh(colors, normals, coefficients, mask=None, normalize=False):
    """The colour G-buffer under spherical-harmonic lighting of the normal G-buffer (colors, normals: [H,W,3] or
    [B,H,W,3], one shape; normals over a -inf background, colors over anything).

    coefficients: [K,3] shared by the frames (its gradient summed over them) or [B,K,3] one set per frame of a batched
    call, K = 1, 4 or 9 (bands 0, 0-1, 0-2); it may require a gradient and stays on the fused path when it does.
    mask ([H,W] or [B,H,W], nonzero = dilate here; None: the pixels where a channel of normals is +-inf, `dilate`'s
    default): the normals are dilated there by `dilate`'s rule.  normalize=True replaces the dilated normal n by
    u = n / (|n| + 1e-12) (diffuse_point's rule for its incident vector, subgradient 0 at n = 0); normalize=False
    uses n raw, as diffuse_directional does.  For a valid pixel, with (x, y, z) that vector:

        c0 = 0.28209479177387814   c1 = 0.4886025119029199   c2 = 1.0925484305920792
        c3 = 0.31539156525252005   c4 = 0.5462742152960396   (as float32 rounds them)
        Y0 = c0          Y1 = c1 y        Y2 = c1 z            Y3 = c1 x
        Y4 = c2 (x y)    Y5 = c2 (y z)    Y6 = c3 (3 z^2 - 1)  Y7 = c2 (x z)    Y8 = c4 (x^2 - y^2)
        E_c = coefficients[0,c] Y0;  E_c = E_c + coefficients[k,c] Y_k for k = 1 .. K-1;  pixels_c = colors_c * E_c

    There is no clamp: an irradiance may go negative, and a caller who wants a clamp applies it to `pixels`.  The
    cosine-lobe factors (pi, 2 pi / 3, pi / 4) are the caller's to fold into the coefficients.

    Returns (pixels, valid): valid [..., H, W, 1] bool marks the pixels whose three dilated normal values are finite;
    the others shade to exactly 0 and carry no gradient.  On the GPU (float32 tensors on one device) the forward is
    one fused launch and the backward two; every gradient is bit-identical from run to run."""
    fn = "shade_sh"
    colors = torch.as_tensor(colors)
    normals = torch.as_tensor(normals, dtype=colors.dtype, device=colors.device)
    if colors.dim() not in (3, 4) or colors.shape[-1] != 3 or normals.shape != colors.shape:
        raise ValueError("%s: colors, normals must share one shape [H, W, 3] or [B, H, W, 3]" % fn)
    if not isinstance(coefficients, torch.Tensor):
        coefficients = torch.as_tensor(coefficients, dtype=colors.dtype, device=colors.device)
    if coefficients.dim() not in (2, 3) or coefficients.shape[-1] != 3:
        raise ValueError("%s: coefficients must be [K, 3] or [B, K, 3]" % fn)
    if coefficients.shape[-2] not in _SH_COUNTS:
        raise ValueError("%s: %d coefficients; K must be 1, 4 or 9 (bands 0, 0-1, 0-2)" % (fn, coefficients.shape[-2]))
    if coefficients.dim() == 3 and (colors.dim() != 4 or coefficients.shape[0] != colors.shape[0]):
        raise ValueError("%s: per-frame coefficients need one set per frame of a [B, H, W, 3] batch" % fn)
    mask = _checked_mask(fn, mask, normals, "normals")
    if (_FUSED_ENABLED and _gpu_f32(colors, normals, coefficients) and
            1 <= min(colors.shape[-3:-1]) and max(colors.shape[-3:-1]) <= _lib.MAX_DIM and
            (mask is None or mask.device == colors.device)):
        (cb, added), (nb, _) = _batched(colors), _batched(normals)
        return _unbatched(_ShadeShFn.apply(cb, nb, coefficients.contiguous(), _kernel_mask(mask, nb),
                                           1 if normalize else 0), added)
    return _shade_sh_ops(colors, normals, coefficients, mask, normalize)


# ---- reflect_view, shade_env: image-based lighting

def _unit_ops(x):
    """x / (|x| + 1e-12) over the last dimension (the length's subgradient at 0 is 0)"""
    length = torch.linalg.norm(x, dim=-1, keepdim=True)
    length = length + 1.e-12
    return x / length


def _per_frame_camera(camera, like):
    """camera [3] or [B,3] as a tensor of like's dtype and device that broadcasts against [...,H,W,3]"""
    camera = torch.as_tensor(camera, dtype=like.dtype, device=like.device)
    return camera[:, None, None, :] if camera.dim() == 2 else camera


def _reflect_view_ops(positions, normals, camera_position):
    """The framework-op statement of reflect_view, each line one operation: positions, normals [H,W,3] or [B,H,W,3],
    camera [3] or [B,3]."""
    pos_s, nrm_s, _, valid = _dilated_gbuffers(positions, positions, normals)
    camera = _per_frame_camera(camera_position, positions)
    n = _unit_ops(nrm_s)
    to_camera = camera - pos_s
    v = _unit_ops(to_camera)
    nv = (n * v).sum(-1, keepdim=True)
    t = 2.0 * nv
    tn = t * n
    directions = tn - v
    return torch.where(valid, directions, 0.0), valid


def _shade_env_ops(positions, colors, normals, material, coefficients, radiance, camera_position, occlusion=None):
    """The framework-op statement of shade_env, each line one operation: G-buffers and radiance [H,W,3] or [B,H,W,3],
    material [...,2], coefficients [K,3] or [B,K,3], camera [3] or [B,3], occlusion [...,1] or None (ones)."""
    dev, dt = positions.device, positions.dtype
    as_t = lambda x: torch.as_tensor(x, dtype=dt, device=dev)  # noqa: E731
    pos_s, nrm_s, col, valid = _dilated_gbuffers(positions, colors, normals)
    mat_s = torch.where(valid, as_t(material), 0.0)
    rad = torch.where(valid, as_t(radiance), 0.0)
    occ = None if occlusion is None else torch.where(valid, as_t(occlusion), 0.0)
    camera = _per_frame_camera(camera_position, positions)
    n = _unit_ops(nrm_s)
    to_camera = camera - pos_s
    v = _unit_ops(to_camera)
    nv = (n * v).sum(-1, keepdim=True)
    nv = nv.clamp_min(0.0)
    r = torch.clamp(mat_s[..., 0:1], _lib.PBR_MIN_ROUGHNESS, 1.0)
    m = torch.clamp(mat_s[..., 1:2], 0.0, 1.0)
    E = _sh_irradiance_ops(n, as_t(coefficients))
    f0 = col - 0.04
    f0 = f0 * m
    f0 = 0.04 + f0
    x = 1.0 - r
    y = 0.0275 * r
    y = 0.0425 - y
    z = 0.572 * r
    z = 1.04 - z
    w = 0.022 * r
    w = w - 0.04
    e = -9.28 * nv
    e = torch.exp2(e)
    q = x * x
    s = torch.where(q < e, q, e)  # (a select: the gradient goes to the chosen side only)
    a = s * x
    a = a + y
    a104 = 1.04 * a
    A = z - a104
    B = a104 + w
    S = f0 * A
    S = S + B
    kd = 1.0 - m
    kd = kd * col
    dif = kd * E
    spec = rad * S
    pixels = dif + spec
    if occ is not None:
        pixels = occ * pixels
    return torch.where(valid, pixels, 0.0), valid


def _valid_outputs(ctx, valid):
    """the kernels' 0 / 1 bytes as the bool `valid` result, which carries no gradient (as the shade's)"""
    valid = valid.view(torch.bool)
    ctx.mark_non_differentiable(valid)
    ctx.set_materialize_grads(False)
    return valid


class _ReflectViewFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, normals, camera):
        B, H, W, _ = positions.shape
        dev = positions.device
        directions = torch.empty_like(positions)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        route = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        cam_pf = 1 if camera.dim() == 2 else 0
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_deferred_reflect_view_fwd(
                positions.data_ptr(), normals.data_ptr(), B, H, W, cam_pf, camera.data_ptr(), directions.data_ptr(),
                valid.data_ptr(), route.data_ptr(), _stream(dev)))
        ctx.save_for_backward(positions, normals, camera, route)
        return directions, _valid_outputs(ctx, valid)

    @staticmethod
    def backward(ctx, grad_directions, _grad_valid):
        _no_double_backward("reflect_view")
        if grad_directions is None:
            return (None,) * 3
        *saved, route = ctx.saved_tensors
        positions, normals, camera = saved
        B, H, W, _ = positions.shape
        dev = positions.device
        grad_directions = grad_directions.contiguous()
        # (NULL for the gradients nobody needs: the kernels then skip them, and without the camera's the partial sums
        # and the second launch as well)
        grads = [torch.empty_like(t) if need else None for t, need in zip(saved, ctx.needs_input_grad[:3])]
        lib = _lib.load()
        workspace, size = None, _lib._SZ(0)
        if grads[2] is not None:
            _lib.check(lib.dirt_deferred_reflect_view_workspace(B, H, W, ctypes.byref(size)))
            workspace = torch.empty((max(size.value, 4),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.dirt_deferred_reflect_view_bwd(
                positions.data_ptr(), normals.data_ptr(), B, H, W, 1 if camera.dim() == 2 else 0, camera.data_ptr(),
                grad_directions.data_ptr(), route.data_ptr(), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]),
                _ptr(workspace), size.value, _stream(dev)))
        return tuple(grads)


def _env_camera(fn, camera_position, positions):
    """camera_position as a tensor ([3] or [B,3], checked)"""
    if not isinstance(camera_position, torch.Tensor):
        camera_position = torch.as_tensor(camera_position, dtype=positions.dtype, device=positions.device)
    frames = positions.shape[0] if positions.dim() == 4 else None
    if tuple(camera_position.shape) not in ((3,), (frames, 3)):
        raise ValueError("%s: camera_position must be [3] or [B, 3]" % fn)
    return camera_position


def _env_dims_fit(positions):
    return 1 <= min(positions.shape[-3:-1]) and max(positions.shape[-3:-1]) <= _lib.MAX_DIM


def reflect_view(positions, normals, camera_position):
    """The reflection of the view vector about the normal, per pixel: the direction `sample_cubemap` and
    `sample_cubemap_mip` look a specular environment up by.

    positions, normals: [H,W,3] or [B,H,W,3] over a -inf background, dilated under the positions' background by
    `shade`'s rule.  camera_position: [3] or [B,3].  For a valid pixel with dilated position p and dilated normal n_d,
    u(x) = x / (|x| + 1e-12) (subgradient 0 at 0):

        n = u(n_d)   v = u(camera - p)   R = (2 n . v) n - v

    n . v is not clamped: a back-facing normal reflects to below the surface.  Returns (directions, valid): valid
    [..., H, W, 1] bool is `shade`'s; an invalid pixel's direction is exactly (0, 0, 0), which both cube-map lookups
    leave out (their `valid` False, texel 0), so the chain needs no mask.

    On the GPU (float32 tensors on one device) the forward is one fused launch and the backward two, whichever of
    positions, normals and the camera need gradients; the camera's is summed in a fixed order: bit-identical from run
    to run."""
    fn = "reflect_view"
    positions = torch.as_tensor(positions)
    normals = torch.as_tensor(normals, dtype=positions.dtype, device=positions.device)
    if positions.dim() not in (3, 4) or positions.shape[-1] != 3 or normals.shape != positions.shape:
        raise ValueError("%s: positions, normals must share one shape [H, W, 3] or [B, H, W, 3]" % fn)
    camera_position = _env_camera(fn, camera_position, positions)
    if _FUSED_ENABLED and _gpu_f32(positions, normals) and _env_dims_fit(positions):
        frames = positions.shape[0] if positions.dim() == 4 else None
        cam = _lights_param(camera_position, positions, ((3,), (frames, 3)))
        if cam is not None:
            (pb, added), (nb, _) = _batched(positions), _batched(normals)
            return _unbatched(_ReflectViewFn.apply(pb, nb, cam), added)
    return _reflect_view_ops(positions, normals, camera_position)


class _ShadeEnvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, colors, normals, material, radiance, occlusion, coefficients, camera):
        B, H, W, _ = positions.shape
        dev = positions.device
        pixels = torch.empty_like(positions)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        route = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        ctx.args = (coefficients.shape[-2], 1 if coefficients.dim() == 3 else 0, 1 if camera.dim() == 2 else 0)
        K, coeffs_pf, cam_pf = ctx.args
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_deferred_shade_env_fwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), material.data_ptr(), radiance.data_ptr(),
                _ptr(occlusion), B, H, W, K, coeffs_pf, coefficients.data_ptr(), cam_pf, camera.data_ptr(),
                pixels.data_ptr(), valid.data_ptr(), route.data_ptr(), _stream(dev)))
        ctx.save_for_backward(positions, colors, normals, material, radiance, occlusion, coefficients, camera, route)
        return pixels, _valid_outputs(ctx, valid)

    @staticmethod
    def backward(ctx, grad_pixels, _grad_valid):
        _no_double_backward("shade_env")
        if grad_pixels is None:
            return (None,) * 8
        *saved, route = ctx.saved_tensors
        positions, colors, normals, material, radiance, occlusion, coefficients, camera = saved
        K, coeffs_pf, cam_pf = ctx.args
        B, H, W, _ = positions.shape
        dev = positions.device
        grad_pixels = grad_pixels.contiguous()
        # (NULL for the gradients nobody needs: the kernels then skip them, and with no parameter among them the
        # partial sums and the second launch as well)
        grads = [torch.empty_like(t) if need and t is not None else None
                 for t, need in zip(saved, ctx.needs_input_grad[:8])]
        lib = _lib.load()
        workspace, size = None, _lib._SZ(0)
        if any(g is not None for g in grads[6:]):
            _lib.check(lib.dirt_deferred_shade_env_workspace(B, H, W, K, ctypes.byref(size)))
            workspace = torch.empty((max(size.value, 4),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.dirt_deferred_shade_env_bwd(
                positions.data_ptr(), colors.data_ptr(), normals.data_ptr(), material.data_ptr(), radiance.data_ptr(),
                _ptr(occlusion), B, H, W, K, coeffs_pf, coefficients.data_ptr(), cam_pf, camera.data_ptr(),
                grad_pixels.data_ptr(), route.data_ptr(), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]),
                _ptr(grads[3]), _ptr(grads[4]), _ptr(grads[5]), _ptr(grads[6]), _ptr(grads[7]), _ptr(workspace),
                size.value, _stream(dev)))
        return tuple(grads)


def shade_env(positions, colors, normals, material, coefficients, radiance, camera_position, occlusion=None):
    """Image-based lighting of a metallic-roughness material by the split-sum approximation: a diffuse irradiance
    environment (spherical harmonics, as `shade_sh`) plus a prefiltered specular environment (`radiance`, usually
    `sample_cubemap_mip` at `reflect_view`'s directions and lod = roughness * (levels - 1)) times the analytic fit of
    the environment BRDF.  `shade_pbr`'s analytic lights add on top.

    positions, colors, normals: the G-buffers, as for `shade_pbr`; colors is the base colour.  material [...,H,W,2]:
    channel 0 the perceptual roughness, channel 1 the metallic.  coefficients: [K,3] shared by the frames or [B,K,3]
    one set per frame, K = 1, 4 or 9, in `shade_sh`'s basis, order and constants; the cosine-lobe factors and any
    1 / pi are the caller's to fold in.  radiance [...,H,W,3].  camera_position: [3] or [B,3].  occlusion: None (ones)
    or [...,H,W,1], an ambient-occlusion factor on both terms.  colors, material, radiance and occlusion are read at
    the pixel itself, never dilated, and are not part of `valid`.

    Dilation of positions and normals, `valid` and the returned (pixels, valid) are `shade`'s.  For a valid pixel with
    dilated position p, dilated normal n_d and colour c, u(x) = x / (|x| + 1e-12):

        n = u(n_d)   v = u(camera - p)   nv = max(n . v, 0)
        r = clamp(material_0, 0.045, 1)   m = clamp(material_1, 0, 1)
        E = coefficients_0 Y_0 + coefficients_1 Y_1(n) + ...         (shade_sh's Y_k and order of additions)
        F0 = 0.04 + (c - 0.04) m
        x = 1 - r   y = 0.0425 - 0.0275 r   z = 1.04 - 0.572 r   w = 0.022 r - 0.04
        e = exp2(-9.28 nv)   q = x^2   s = min(q, e), the gradient to the chosen side only
        a = s x + y          A = z - 1.04 a          B = 1.04 a + w
        pixels = occlusion (((1 - m) c) E + radiance (F0 A + B))

    B may reach about -0.0024 at r = 1; there is no clamp.  Every clamp takes torch.clamp's derivative, so a roughness
    below 0.045 receives a zero gradient; max(., 0) passes the gradient where its argument is >= 0.

    On the GPU (float32 tensors on one device) the forward is one fused launch and the backward two, whichever inputs
    need gradients: the G-buffers, the material, the radiance, the occlusion, the coefficients and the camera.  A
    parameter's gradient is the sum of its per-pixel terms in a fixed order: bit-identical from run to run."""
    fn = "shade_env"
    positions, colors, normals = _gbuffers(fn, positions, colors, normals)
    dev, dt = positions.device, positions.dtype
    as_t = lambda x: x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=dt, device=dev)  # noqa: E731
    material, radiance, coefficients = as_t(material), as_t(radiance), as_t(coefficients)
    if material.shape != positions.shape[:-1] + (2,):
        raise ValueError("%s: material of shape %s for positions of shape %s; it must be [..., H, W, 2]"
                         % (fn, tuple(material.shape), tuple(positions.shape)))
    if radiance.shape != positions.shape:
        raise ValueError("%s: radiance of shape %s for positions of shape %s; it must be [..., H, W, 3]"
                         % (fn, tuple(radiance.shape), tuple(positions.shape)))
    if occlusion is not None:
        occlusion = as_t(occlusion)
        if occlusion.shape != positions.shape[:-1] + (1,):
            raise ValueError("%s: occlusion of shape %s for positions of shape %s; it must be [..., H, W, 1]"
                             % (fn, tuple(occlusion.shape), tuple(positions.shape)))
    if coefficients.dim() not in (2, 3) or coefficients.shape[-1] != 3:
        raise ValueError("%s: coefficients must be [K, 3] or [B, K, 3]" % fn)
    K = coefficients.shape[-2]
    if K not in _SH_COUNTS:
        raise ValueError("%s: %d coefficients; K must be 1, 4 or 9 (bands 0, 0-1, 0-2)" % (fn, K))
    frames = positions.shape[0] if positions.dim() == 4 else None
    if coefficients.dim() == 3 and coefficients.shape[0] != frames:
        raise ValueError("%s: per-frame coefficients need one set per frame of a [B, H, W, 3] batch" % fn)
    camera_position = _env_camera(fn, camera_position, positions)
    if _FUSED_ENABLED and _gpu_f32(positions, colors, normals, material, radiance) and _env_dims_fit(positions) and \
            (occlusion is None or _gpu_f32(positions, occlusion)):
        coef = _lights_param(coefficients, positions, ((K, 3), (frames, K, 3)))
        cam = _lights_param(camera_position, positions, ((3,), (frames, 3)))
        if coef is not None and cam is not None:
            ops, added = zip(*(_batched(x) for x in (positions, colors, normals, material, radiance)))
            occ = None if occlusion is None else _batched(occlusion)[0]
            return _unbatched(_ShadeEnvFn.apply(*ops, occ, coef, cam), added[0])
    return _shade_env_ops(positions, colors, normals, material, coefficients, radiance, camera_position, occlusion)


# ---- texture sampling

_WRAPS ={"clamp": _lib.TEXTURE_CLAMP, "repeat": _lib.TEXTURE_REPEAT}


def _texture_axis(u, T, wrap):
    """One coordinate of the sampling rule: (first tap, second tap, weight of the second), each line one operation.
    The taps are reduced into [0, T) before they index anything; floor has derivative 0."""
    uc = u - torch.floor(u) if wrap == "repeat" else torch.clamp(u, 0.0, 1.0)
    x = uc * T
    x = x - 0.5
    fx = torch.floor(x).detach()
    a = x - fx
    # fx is in [-1, T - 1] for every finite u; a NaN goes to -1, so the conversion is defined for any u
    j0 = torch.where(fx >= 0, torch.clamp(fx, max=T), -1.0).to(torch.int64)
    j1 = j0 + 1
    if wrap == "repeat":
        return torch.remainder(j0, T), torch.remainder(j1, T), a
    return torch.clamp(j0, 0, T - 1), torch.clamp(j1, 0, T - 1), a


def _gather_taps(texture, uv, sampled, wrap):
    """The four taps ([...,C]) of the pixels in `sampled` and the weights of the second column and row ([...,1]):
    (t00, t01, t10, t11, a, b); texture [Th,Tw,C] or [B,Th,Tw,C]."""
    Th, Tw = texture.shape[-3], texture.shape[-2]
    uvs = torch.where(sampled[..., None], uv, 0.0)  # (no index is ever formed from an unsampled pixel's uv)
    j0, j1, a = _texture_axis(uvs[..., 0], Tw, wrap)
    i0, i1, b = _texture_axis(uvs[..., 1], Th, wrap)
    if texture.dim() == 4:
        f = torch.arange(texture.shape[0], device=texture.device)[:, None, None]
        taps = texture[f, i0, j0], texture[f, i0, j1], texture[f, i1, j0], texture[f, i1, j1]
    else:
        taps = texture[i0, j0], texture[i0, j1], texture[i1, j0], texture[i1, j1]
    return taps + (a[..., None], b[..., None])


def _sample_texture_ops(texture, uv, mask=None, wrap="clamp"):
    """texture [Th,Tw,C] or [B,Th,Tw,C], uv [H,W,2] or [B,H,W,2], mask (uv's shape without the channels) or None."""
    valid = torch.isfinite(uv).all(-1) if mask is None else mask != 0
    t00, t01, t10, t11, a, b = _gather_taps(texture, uv, valid, wrap)
    oma, omb = 1.0 - a, 1.0 - b
    top = t00 * oma + t01 * a
    bot = t10 * oma + t11 * a
    out = top * omb + bot * b
    return torch.where(valid[..., None], out, 0.0), valid[..., None]


class _SampleTextureFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, uv, mask, wrap):
        Tf, Th, Tw, C = texture.shape
        B, H, W, _ = uv.shape
        dev = uv.device
        texels = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_fwd(texture.data_ptr(), Tf, Th, Tw, C, uv.data_ptr(), _ptr(mask),
                                                           B, H, W, wrap, texels.data_ptr(), valid.data_ptr(),
                                                           _stream(dev)))
        ctx.save_for_backward(texture, uv, mask)
        ctx.wrap = wrap
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # (as the shade: no zero-filled "gradient" of valid)
        return texels, valid

    @staticmethod
    def backward(ctx, grad_texels, _grad_valid):
        _no_double_backward("sample_texture")
        if grad_texels is None:
            return None, None, None, None
        texture, uv, mask = ctx.saved_tensors
        Tf, Th, Tw, C = texture.shape
        B, H, W, _ = uv.shape
        dev = uv.device
        grad_texels = grad_texels.contiguous()
        # (NULL for the gradient nobody needs: the kernel then skips it; grad_texture is zero-filled by the call)
        grad_texture = torch.empty_like(texture) if ctx.needs_input_grad[0] else None
        grad_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_bwd(texture.data_ptr(), Tf, Th, Tw, C, uv.data_ptr(), _ptr(mask),
                                                           B, H, W, ctx.wrap, grad_texels.data_ptr(),
                                                           _ptr(grad_texture), _ptr(grad_uv), _stream(dev)))
        return grad_texture, grad_uv, None, None


def sample_texture(texture, uv, mask=None, wrap="clamp"):
    """Bilinear lookup of texture ([Th,Tw,C]: shared by every frame, its gradient sums over them; or [B,Th,Tw,C]: one
    per frame) at uv ([H,W,2] or [B,H,W,2]; u along the texture's width, v along its height, top row first; texel
    (i,j) has its centre at u = (j + 0.5) / Tw, v = (i + 0.5) / Th).  wrap is "clamp" (GL CLAMP_TO_EDGE) or "repeat".
    A pixel is sampled where mask ([H,W] or [B,H,W]) is nonzero; mask=None samples the pixels whose two uv channels
    are finite, so a uv G-buffer rendered over a -inf background needs no mask.

    Returns (texels, valid): valid [..., H, W, 1] bool marks the sampled pixels and carries no gradient; the others
    give exactly 0 and carry no gradient.  The uv gradient follows torch.clamp at 0 and 1 (clamp mode) and takes
    floor's derivative as 0; on the GPU it is bit-identical from run to run, while the texture gradient is summed with
    float atomics and may differ in the last bits."""
    texture = torch.as_tensor(texture)
    uv = torch.as_tensor(uv, dtype=texture.dtype, device=texture.device)
    if wrap not in _WRAPS:
        raise ValueError("sample_texture: wrap must be 'clamp' or 'repeat', not %r" % (wrap,))
    if uv.dim() not in (3, 4) or uv.shape[-1] != 2:
        raise ValueError("sample_texture: uv must be [H, W, 2] or [B, H, W, 2]")
    if texture.dim() not in (3, 4) or min(texture.shape[-3:]) < 1:
        raise ValueError("sample_texture: texture must be a non-empty [Th, Tw, C] or [B, Th, Tw, C]")
    if texture.dim() == 4 and (uv.dim() != 4 or texture.shape[0] != uv.shape[0]):
        raise ValueError("sample_texture: a per-frame texture of shape %s for uv of shape %s"
                         % (tuple(texture.shape), tuple(uv.shape)))
    mask = _checked_mask("sample_texture", mask, uv, "uv")
    if (_FUSED_ENABLED and _gpu_f32(texture, uv) and 1 <= texture.shape[-1] <= _lib.MAX_CHANNELS and
            max(texture.shape[-3], texture.shape[-2]) <= _lib.MAX_DIM and
            1 <= min(uv.shape[-3:-1]) and max(uv.shape[-3:-1]) <= _lib.MAX_DIM and
            (mask is None or mask.device == uv.device)):
        (tb, _), (ub, added) = _batched(texture), _batched(uv)
        return _unbatched(_SampleTextureFn.apply(tb, ub, _kernel_mask(mask, ub), _WRAPS[wrap]), added)
    return _sample_texture_ops(texture, uv, mask, wrap)


# ---- mipmapped texture sampling

def _mip_dims(Th, Tw, levels=None):
    """[(Th_k, Tw_k)] of the chain: level k + 1 exists while level k has every dimension even or 1 and not both 1."""
    dims = [(int(Th), int(Tw))]
    while levels is None or len(dims) < levels:
        h, w = dims[-1]
        if (h == 1 and w == 1) or (h > 1 and h % 2) or (w > 1 and w % 2):
            break
        dims.append((max(1, h // 2), max(1, w // 2)))
    return dims


class Mipmaps:
    """A packed mip chain: `packed` [N,C] (shared by the frames) or [B,N,C] (one per frame), N = sum_k Th_k * Tw_k, the
    levels in order, each row-major; `dims` = ((Th_0, Tw_0), ...); `level(k)` a [..., Th_k, Tw_k, C] view of packed;
    len() the number of levels.  build_mipmaps makes the box-filtered chain; Mipmaps(packed, Th, Tw, levels) wraps a
    chain filtered any other way (levels=None: the whole chain of a Th x Tw texture)."""

    def __init__(self, packed, Th, Tw, levels=None):
        packed = torch.as_tensor(packed)
        if levels is not None and (int(levels) != levels or levels < 1):
            raise ValueError("Mipmaps: levels must be a positive integer or None")
        if Th < 1 or Tw < 1:
            raise ValueError("Mipmaps: the texture must be non-empty")
        dims = _mip_dims(Th, Tw, levels)
        if levels is not None and len(dims) != levels:
            raise ValueError("Mipmaps: levels = %d, but the chain of a %d x %d texture has %d"
                             % (levels, Th, Tw, len(dims)))
        n = sum(h * w for h, w in dims)
        if packed.dim() not in (2, 3) or packed.shape[-2] != n or packed.shape[-1] < 1 or packed.shape[0] < 1:
            raise ValueError("Mipmaps: packed must be [N, C] or [B, N, C] with N = %d for %d levels of a %d x %d "
                             "texture, not %s" % (n, len(dims), Th, Tw, tuple(packed.shape)))
        self.packed, self.dims = packed, tuple(dims)
        self.offsets = tuple(sum(h * w for h, w in dims[:k]) for k in range(len(dims)))

    def __len__(self):
        return len(self.dims)

    def level(self, k):
        (h, w), o = self.dims[k], self.offsets[k]
        return self.packed[..., o:o + h * w, :].unflatten(-2, (h, w))


def _build_mipmaps_ops(texture, levels=None):
    """texture [Th,Tw,C] or [B,Th,Tw,C] -> Mipmaps; each level the pairwise tree of the rule, one operation a line."""
    dims = _mip_dims(texture.shape[-3], texture.shape[-2], levels)
    chain = [texture]
    for h, w in dims[:-1]:
        t = chain[-1]
        if h >= 2 and w >= 2:
            top = t[..., 0::2, 0::2, :] + t[..., 0::2, 1::2, :]
            bot = t[..., 1::2, 0::2, :] + t[..., 1::2, 1::2, :]
            chain.append((top + bot) * 0.25)
        elif w >= 2:
            chain.append((t[..., :, 0::2, :] + t[..., :, 1::2, :]) * 0.5)
        else:
            chain.append((t[..., 0::2, :, :] + t[..., 1::2, :, :]) * 0.5)
    packed = torch.cat([t.flatten(-3, -2) for t in chain], -2)
    return Mipmaps(packed, dims[0][0], dims[0][1], len(dims))


class _BuildMipmapsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, levels):
        Tf, Th, Tw, C = texture.shape
        n = sum(h * w for h, w in _mip_dims(Th, Tw, levels))
        packed = torch.empty((Tf, n, C), dtype=torch.float32, device=texture.device)
        with torch.cuda.device(texture.device):
            _lib.check(_lib.load().dirt_texture_mip_build_fwd(texture.data_ptr(), Tf, Th, Tw, C, levels,
                                                              packed.data_ptr(), _stream(texture.device)))
        ctx.shape, ctx.levels = texture.shape, levels
        return packed

    @staticmethod
    def backward(ctx, grad_packed):
        _no_double_backward("build_mipmaps")
        Tf, Th, Tw, C = ctx.shape
        grad_packed = grad_packed.contiguous()
        grad_texture = torch.empty(ctx.shape, dtype=torch.float32, device=grad_packed.device)
        with torch.cuda.device(grad_packed.device):
            _lib.check(_lib.load().dirt_texture_mip_build_bwd(grad_packed.data_ptr(), Tf, Th, Tw, C, ctx.levels,
                                                              grad_texture.data_ptr(), _stream(grad_packed.device)))
        return grad_texture, None


def _mip_fused_texture(shape):
    """the kernels' limits on a texture [..., Th, Tw, C]"""
    return 1 <= shape[-1] <= _lib.MAX_CHANNELS and max(shape[-3], shape[-2]) <= _lib.MAX_DIM


def build_mipmaps(texture, levels=None):
    """The box-filtered mip chain of texture ([Th,Tw,C] or [B,Th,Tw,C]) as a Mipmaps, differentiable to the texture.
    Level k + 1 halves level k (each texel the mean of its 2 x 2 block, of its pair where one dimension is 1) while
    every dimension of level k is even or 1 and not both are 1: an odd dimension > 1 ends the chain (5 x 7: one level,
    6 x 10: two, 64 x 64: seven).  levels=n keeps at most the first n levels."""
    texture = torch.as_tensor(texture)
    if texture.dim() not in (3, 4) or min(texture.shape) < 1:
        raise ValueError("build_mipmaps: texture must be a non-empty [Th, Tw, C] or [B, Th, Tw, C]")
    if levels is not None and (not isinstance(levels, int) or levels < 1):
        raise ValueError("build_mipmaps: levels must be a positive integer or None")
    if _FUSED_ENABLED and _gpu_f32(texture) and _mip_fused_texture(texture.shape):
        dims = _mip_dims(texture.shape[-3], texture.shape[-2], levels)
        tb, added = _batched(texture)
        return Mipmaps(_unbatched(_BuildMipmapsFn.apply(tb, len(dims)), added), dims[0][0], dims[0][1], len(dims))
    return _build_mipmaps_ops(texture, levels)


def _mip_difference(uv, valid, dim):
    """The rule's difference of uv ([...,H,W,2]) along dim (-3: y, -2: x): to the next pixel where there is one and it
    is sampled, else from the previous one where there is one and it is sampled, else 0."""
    n = uv.shape[dim]
    if n == 1:
        return torch.zeros_like(uv)
    step = uv.narrow(dim, 1, n - 1) - uv.narrow(dim, 0, n - 1)  # step[i] = uv[i + 1] - uv[i]
    zero = torch.zeros_like(uv.narrow(dim, 0, 1))
    no = torch.zeros_like(valid.narrow(dim + 1, 0, 1))
    use_next = torch.cat([valid.narrow(dim + 1, 1, n - 1), no], dim + 1)[..., None]
    use_prev = torch.cat([no, valid.narrow(dim + 1, 0, n - 1)], dim + 1)[..., None]
    return torch.where(use_next, torch.cat([step, zero], dim),
                       torch.where(use_prev, torch.cat([zero, step], dim), torch.zeros_like(uv)))


def _mip_lod_of_rho2(rho2, L):
    """The rule's piecewise-linear 0.5 * log2(rho2): 0 unless rho2 >= 1, L - 1 at inf."""
    m, e = torch.frexp(torch.where(torch.isfinite(rho2), rho2, 1.0))  # rho2 = m * 2^e, m in [0.5, 1)
    lod = 0.5 * ((e - 1).to(rho2.dtype) + (m * 2.0 - 1.0))
    lod = torch.where(rho2 >= 1.0, lod, 0.0)
    return torch.where(torch.isinf(rho2), float(L - 1), lod)


def _mip_lod_ops(uv, valid, Th, Tw, L, lod=None, lod_bias=0.0):
    """The final level of detail [...,H,W] of the rule (0 at unsampled pixels), detached: it carries no gradient."""
    uv = uv.detach()
    if lod is None:
        q = []
        for dim in (-2, -3):
            d = _mip_difference(uv, valid, dim)
            du = d[..., 0] * Tw
            dv = d[..., 1] * Th
            q.append(du * du + dv * dv)
        lod = _mip_lod_of_rho2(torch.fmax(q[0], q[1]), L)  # (a NaN loses against a number)
    else:
        lod = lod.detach().to(uv.dtype)
        lod = torch.where(torch.isnan(lod), 0.0, lod)
    lod = lod + lod_bias
    lod = torch.clamp(lod, 0.0, float(L - 1))
    return torch.where(valid, lod, 0.0)


class _BilinearFn(torch.autograd.Function):
    """The bilinear rule on four gathered taps ([...,C]) and the two weights ([...,1]), each line one operation.  Its
    backward takes the weights' gradients in the kernels' difference form,
        grad_a = sum_c g_c * ((t01 - t00) * (1 - b) + (t11 - t10) * b),   grad_b = sum_c g_c * (bot_c - top_c),
    so that a float32 gradient rounds texel differences, as the statement's bound counts, where plain autograd rounds
    differences of products.  The backward is itself framework ops on the saved inputs: it differentiates again, with
    every second derivative (the mixed one in a and b, and those between the weights and the taps)."""

    @staticmethod
    def forward(ctx, t00, t01, t10, t11, a, b):
        ctx.save_for_backward(t00, t01, t10, t11, a, b)
        oma, omb = 1.0 - a, 1.0 - b
        top = t00 * oma + t01 * a
        bot = t10 * oma + t11 * a
        return top * omb + bot * b

    @staticmethod
    def backward(ctx, g):
        t00, t01, t10, t11, a, b = ctx.saved_tensors
        oma, omb = 1.0 - a, 1.0 - b
        g_top, g_bot = g * omb, g * b
        du = (t01 - t00) * omb + (t11 - t10) * b
        top = t00 * oma + t01 * a
        bot = t10 * oma + t11 * a
        grad_a = (g * du).sum(-1, keepdim=True)
        grad_b = (g * (bot - top)).sum(-1, keepdim=True)
        return g_top * oma, g_top * a, g_bot * oma, g_bot * a, grad_a, grad_b


def _mip_level_ops(texture, uv, sampled, wrap):
    """`_sample_texture_ops`' rule at one level, for the pixels in `sampled`; the value is the rule's bit for bit, the
    uv gradient is in the kernels' difference form (`_BilinearFn`), and it differentiates again."""
    out = _BilinearFn.apply(*_gather_taps(texture, uv, sampled, wrap))
    return torch.where(sampled[..., None], out, 0.0)


def _sample_texture_mip_ops(mipmaps, uv, mask=None, wrap="clamp", lod=None, lod_bias=0.0):
    """mipmaps a Mipmaps, uv [H,W,2] or [B,H,W,2], mask and lod (uv's shape without the channels) or None
    -> (texels, valid, the final lod)."""
    (Th, Tw), L = mipmaps.dims[0], len(mipmaps)
    valid = torch.isfinite(uv).all(-1) if mask is None else mask != 0
    lod = _mip_lod_ops(uv, valid, Th, Tw, L, lod, lod_bias)
    k0f = torch.floor(lod)
    f = (lod - k0f)[..., None]
    k0 = k0f.to(torch.int64)
    k1 = torch.clamp(k0 + 1, max=L - 1)
    blend = valid & (f[..., 0] != 0)
    s0 = torch.zeros(uv.shape[:-1] + (mipmaps.packed.shape[-1],), dtype=uv.dtype, device=uv.device)
    s1 = s0
    for k in range(L):  # (a level is read only by the pixels that the rule sends there)
        at0, at1 = valid & (k0 == k), blend & (k1 == k)
        if not bool((at0 | at1).any()):
            continue
        s = _mip_level_ops(mipmaps.level(k), uv, at0 | at1, wrap)
        s0 = torch.where(at0[..., None], s, s0)
        s1 = torch.where(at1[..., None], s, s1)
    out = torch.where(blend[..., None], s0 * (1.0 - f) + s1 * f, s0)
    return torch.where(valid[..., None], out, 0.0), valid[..., None], lod


class _SampleTextureMipFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed, uv, mask, lod_in, Th, Tw, levels, wrap, lod_bias):
        Tf, _, C = packed.shape
        B, H, W, _ = uv.shape
        dev = uv.device
        texels = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        lod = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_mip_fwd(
                packed.data_ptr(), Tf, Th, Tw, C, levels, uv.data_ptr(), _ptr(mask), _ptr(lod_in), lod_bias, B, H, W,
                wrap, texels.data_ptr(), valid.data_ptr(), lod.data_ptr(), _stream(dev)))
        ctx.save_for_backward(packed, uv, mask, lod)
        ctx.args = (Th, Tw, levels, wrap)
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid, lod)
        ctx.set_materialize_grads(False)  # (as sample_texture: no zero-filled "gradient" of valid or the lod)
        return texels, valid, lod

    @staticmethod
    def backward(ctx, grad_texels, _grad_valid, _grad_lod):
        _no_double_backward("sample_texture_mip")
        if grad_texels is None:
            return (None,) * 9
        packed, uv, mask, lod = ctx.saved_tensors
        Th, Tw, levels, wrap = ctx.args
        Tf, _, C = packed.shape
        B, H, W, _ = uv.shape
        dev = uv.device
        grad_texels = grad_texels.contiguous()
        # (NULL for the gradient nobody needs: the kernel then skips it; grad_packed is zero-filled by the call)
        grad_packed = torch.empty_like(packed) if ctx.needs_input_grad[0] else None
        grad_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_mip_bwd(
                packed.data_ptr(), Tf, Th, Tw, C, levels, uv.data_ptr(), _ptr(mask), lod.data_ptr(), B, H, W, wrap,
                grad_texels.data_ptr(), _ptr(grad_packed), _ptr(grad_uv), _stream(dev)))
        return (grad_packed, grad_uv) + (None,) * 7


def _sample_texture_mip(mipmaps, uv, mask=None, wrap="clamp", lod=None, lod_bias=0.0):
    """sample_texture_mip with the pixels' final lod as a third result (the buffer the fused backward reads)."""
    fn = "sample_texture_mip"
    if not isinstance(mipmaps, Mipmaps):
        mipmaps = build_mipmaps(mipmaps)
    packed = mipmaps.packed
    uv = torch.as_tensor(uv, dtype=packed.dtype, device=packed.device)
    if wrap not in _WRAPS:
        raise ValueError("%s: wrap must be 'clamp' or 'repeat', not %r" % (fn, wrap))
    if uv.dim() not in (3, 4) or uv.shape[-1] != 2:
        raise ValueError("%s: uv must be [H, W, 2] or [B, H, W, 2]" % fn)
    if packed.dim() == 3 and (uv.dim() != 4 or packed.shape[0] != uv.shape[0]):
        raise ValueError("%s: a per-frame chain of shape %s for uv of shape %s"
                         % (fn, tuple(packed.shape), tuple(uv.shape)))
    mask = _checked_mask(fn, mask, uv, "uv")
    if lod is not None:
        lod = torch.as_tensor(lod, device=uv.device)
        if lod.shape != uv.shape[:-1] or not lod.is_floating_point():
            raise ValueError("%s: lod must be a float tensor of shape %s, not %s"
                             % (fn, tuple(uv.shape[:-1]), tuple(lod.shape)))
    if isinstance(lod_bias, torch.Tensor) or not float("-inf") < float(lod_bias) < float("inf"):
        raise ValueError("%s: lod_bias must be a finite number" % fn)
    lod_bias = float(lod_bias)
    (Th, Tw), L = mipmaps.dims[0], len(mipmaps)
    if (_FUSED_ENABLED and _gpu_f32(packed, uv) and _mip_fused_texture((Th, Tw, packed.shape[-1])) and
            L <= _lib.MAX_MIP_LEVELS and 1 <= min(uv.shape[-3:-1]) and max(uv.shape[-3:-1]) <= _lib.MAX_DIM and
            (mask is None or mask.device == uv.device)):
        (pb, _), (ub, added) = _batched(packed, 3), _batched(uv)
        lb = None if lod is None else lod.detach().to(torch.float32).contiguous().reshape(ub.shape[:-1])
        return _unbatched(_SampleTextureMipFn.apply(pb, ub, _kernel_mask(mask, ub), lb, Th, Tw, L, _WRAPS[wrap],
                                                    lod_bias), added)
    return _sample_texture_mip_ops(mipmaps, uv, mask, wrap, lod, lod_bias)


def sample_texture_mip(mipmaps, uv, mask=None, wrap="clamp", lod=None, lod_bias=0.0):
    """Trilinear lookup of a mip chain (a Mipmaps, or a plain texture [Th,Tw,C] / [B,Th,Tw,C] whose chain is built
    inside the call) at uv, with sample_texture's conventions for uv, mask, wrap and the two results (texels, valid).

    Each sampled pixel takes its level of detail from the uv differences to its sampled neighbours (the next pixel in
    x and in y where there is one, else the previous one, else 0), scaled to texels: rho2 = max(|d_x|^2, |d_y|^2),
    lod = 0.5 * (e + m - 1) for rho2 = m * 2^e with m in [1, 2) -- log2 made piecewise linear, exact at powers of two;
    0 for rho2 < 1.  lod ([H,W] or [B,H,W]) replaces that (a NaN in it counts as 0).  lod_bias is added, the sum
    clamped to [0, levels - 1], and the result is sample_texture at level floor(lod) blended with the next level by
    the fractional part (an integer lod reads one level only).

    The lod carries no gradient: neither uv (through the differences) nor an explicit lod receives one from it.  The
    uv gradient is the blend of the two levels' sample_texture gradients; the gradient to the chain, and through
    build_mipmaps to the texture, reaches every texel under a minified pixel's footprint.  On the GPU the uv gradient
    and build_mipmaps' backward are bit-identical from run to run; the chain's gradient is summed with float atomics."""
    return _sample_texture_mip(mipmaps, uv, mask, wrap, lod, lod_bias)[:2]


# ---- cube-map sampling

def _cube_coordinates(directions, sampled):
    """The face rule, each line one operation: (face int64, u, v) of the pixels in `sampled`; the others take the
    direction (1, 1, 1), so that no index and no NaN is formed from theirs.  The face choice has derivative 0."""
    d = torch.where(sampled[..., None], directions, 1.0)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = x.abs(), y.abs(), z.abs()
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    ma = torch.where(is_x, x, torch.where(is_y, y, z))
    neg = ma < 0  # (-0.0 takes the positive face)
    face = torch.where(is_x, 0, torch.where(is_y, 2, 4)) + neg.to(torch.int64)
    sc = torch.where(is_x, torch.where(neg, z, -z), torch.where(is_y, x, torch.where(neg, -x, x)))
    tc = torch.where(is_y, torch.where(neg, -z, z), -y)
    m = ma.abs()
    su = sc / m
    sv = tc / m
    u = su + 1.0
    u = u * 0.5
    v = sv + 1.0
    v = v * 0.5
    return face, u, v


def _sample_cubemap_ops(cubemap, directions, mask=None):
    """cubemap [6,S,S,C] or [B,6,S,S,C], directions [H,W,3] or [B,H,W,3], mask (directions' shape without the
    channels) or None."""
    valid = torch.isfinite(directions).all(-1) & (directions != 0).any(-1)
    if mask is not None:
        valid = valid & (mask != 0)
    S = cubemap.shape[-2]
    face, u, v = _cube_coordinates(directions, valid)
    j0, j1, a = _texture_axis(u, S, "clamp")
    i0, i1, b = _texture_axis(v, S, "clamp")
    if cubemap.dim() == 5:
        f = torch.arange(cubemap.shape[0], device=cubemap.device)[:, None, None]
        t00, t01, t10, t11 = cubemap[f, face, i0, j0], cubemap[f, face, i0, j1], cubemap[f, face, i1, j0], \
            cubemap[f, face, i1, j1]
    else:
        t00, t01, t10, t11 = cubemap[face, i0, j0], cubemap[face, i0, j1], cubemap[face, i1, j0], cubemap[face, i1, j1]
    a, b = a[..., None], b[..., None]
    oma, omb = 1.0 - a, 1.0 - b
    top = t00 * oma + t01 * a
    bot = t10 * oma + t11 * a
    out = top * omb + bot * b
    return torch.where(valid[..., None], out, 0.0), valid[..., None]


class _SampleCubemapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap, directions, mask):
        Cf, _, S, _, C = cubemap.shape
        B, H, W, _ = directions.shape
        dev = directions.device
        texels = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_cube_fwd(cubemap.data_ptr(), Cf, S, C, directions.data_ptr(),
                                                                _ptr(mask), B, H, W, texels.data_ptr(),
                                                                valid.data_ptr(), _stream(dev)))
        ctx.save_for_backward(cubemap, directions, mask)
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # (as the shade: no zero-filled "gradient" of valid)
        return texels, valid

    @staticmethod
    def backward(ctx, grad_texels, _grad_valid):
        _no_double_backward("sample_cubemap")
        if grad_texels is None:
            return None, None, None
        cubemap, directions, mask = ctx.saved_tensors
        Cf, _, S, _, C = cubemap.shape
        B, H, W, _ = directions.shape
        dev = directions.device
        grad_texels = grad_texels.contiguous()
        # (NULL for the gradient nobody needs: the kernel then skips it; grad_cubemap is zero-filled by the call)
        grad_cubemap = torch.empty_like(cubemap) if ctx.needs_input_grad[0] else None
        grad_directions = torch.empty_like(directions) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_cube_bwd(cubemap.data_ptr(), Cf, S, C, directions.data_ptr(),
                                                                _ptr(mask), B, H, W, grad_texels.data_ptr(),
                                                                _ptr(grad_cubemap), _ptr(grad_directions),
                                                                _stream(dev)))
        return grad_cubemap, grad_directions, None


def sample_cubemap(cubemap, directions, mask=None):
    """Bilinear lookup of cubemap ([6,S,S,C]: shared by every frame, its gradient sums over them; or [B,6,S,S,C]: one
    per frame) at directions ([H,W,3] or [B,H,W,3]; they need not be unit length).  The faces are square, in the order
    +x, -x, +y, -y, +z, -z, each laid out as sample_texture's texture: top row first, texel (i,j) centred at
    u = (j + 0.5) / S, v = (i + 0.5) / S.  With (x, y, z) a direction:

        major axis: x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z; ma is that component, and the face
        is the negative one exactly when ma < 0.  (sc, tc) by the OpenGL table:
          +x: (-z, -y)   -x: (+z, -y)   +y: (+x, +z)   -y: (+x, -z)   +z: (+x, -y)   -z: (-x, -y)
        u = (sc / |ma| + 1) * 0.5,  v = (tc / |ma| + 1) * 0.5

    and the face is filtered at (u, v) as sample_texture filters a texture with wrap="clamp".  Filtering clamps to the
    face's edge: there is no filtering across face seams; sample_cubemap_mip filters across them, at every level.

    A pixel is sampled where mask ([H,W] or [B,H,W]) is nonzero (mask=None: everywhere) and its direction's three
    values are finite and not all zero, so a direction G-buffer rendered over -inf needs no mask, and a mask never
    makes a zero or non-finite direction form an address.

    Returns (texels, valid): valid [..., H, W, 1] bool marks the sampled pixels and carries no gradient; the others
    give exactly 0 and carry no gradient.  The directions' gradient takes the derivative of the face choice and of
    floor as 0, and is orthogonal to the direction (the lookup does not depend on its length); on the GPU it is
    bit-identical from run to run, while the cube map's gradient is summed with float atomics and may differ in the
    last bits."""
    fn = "sample_cubemap"
    cubemap = torch.as_tensor(cubemap)
    directions = torch.as_tensor(directions, dtype=cubemap.dtype, device=cubemap.device)
    if directions.dim() not in (3, 4) or directions.shape[-1] != 3:
        raise ValueError("%s: directions must be [H, W, 3] or [B, H, W, 3]" % fn)
    if cubemap.dim() not in (4, 5) or cubemap.shape[-4] != 6:
        raise ValueError("%s: cubemap must be [6, S, S, C] or [B, 6, S, S, C], not %s" % (fn, tuple(cubemap.shape)))
    if cubemap.shape[-3] != cubemap.shape[-2] or min(cubemap.shape[-2:]) < 1:
        raise ValueError("%s: the faces must be square and non-empty, not %s" % (fn, tuple(cubemap.shape[-3:])))
    if cubemap.dim() == 5 and (directions.dim() != 4 or cubemap.shape[0] != directions.shape[0]):
        raise ValueError("%s: a per-frame cubemap of shape %s for directions of shape %s"
                         % (fn, tuple(cubemap.shape), tuple(directions.shape)))
    mask = _checked_mask(fn, mask, directions, "directions")
    if (_FUSED_ENABLED and _gpu_f32(cubemap, directions) and 1 <= cubemap.shape[-1] <= _lib.MAX_CHANNELS and
            cubemap.shape[-2] <= _lib.MAX_DIM and
            1 <= min(directions.shape[-3:-1]) and max(directions.shape[-3:-1]) <= _lib.MAX_DIM and
            (mask is None or mask.device == directions.device)):
        (cb, _), (db, added) = _batched(cubemap, 5), _batched(directions)
        return _unbatched(_SampleCubemapFn.apply(cb, db, _kernel_mask(mask, db)), added)
    return _sample_cubemap_ops(cubemap, directions, mask)


# ---- seamless mip-mapped cube-map sampling

class CubeMipmaps:
    """A cube map's packed mip chain: `packed` [6,N,C] (shared by the frames) or [B,6,N,C] (one per frame), face-major,
    each face's chain as a Mipmaps packs it (N = sum_k S_k^2, S_k = S >> k while S_k is even); `dims` = ((S_0, S_0),
    ...); `level(k)` a [..., 6, S_k, S_k, C] view of packed; len() the number of levels.  build_cubemap_mipmaps makes
    the box-filtered chain; CubeMipmaps(packed, S, levels) wraps a chain filtered any other way (a GGX prefilter, say;
    levels=None: the whole chain of S x S faces)."""

    def __init__(self, packed, S, levels=None):
        packed = torch.as_tensor(packed)
        if levels is not None and (int(levels) != levels or levels < 1):
            raise ValueError("CubeMipmaps: levels must be a positive integer or None")
        if S < 1:
            raise ValueError("CubeMipmaps: the faces must be non-empty")
        dims = _mip_dims(S, S, levels)
        if levels is not None and len(dims) != levels:
            raise ValueError("CubeMipmaps: levels = %d, but the chain of %d x %d faces has %d"
                             % (levels, S, S, len(dims)))
        n = sum(h * w for h, w in dims)
        if packed.dim() not in (3, 4) or packed.shape[-3] != 6 or packed.shape[-2] != n or packed.shape[-1] < 1 or \
                packed.shape[0] < 1:
            raise ValueError("CubeMipmaps: packed must be [6, N, C] or [B, 6, N, C] with N = %d for %d levels of "
                             "%d x %d faces, not %s" % (n, len(dims), S, S, tuple(packed.shape)))
        self.packed, self.dims = packed, tuple(dims)
        self.offsets = tuple(sum(h * w for h, w in dims[:k]) for k in range(len(dims)))

    def __len__(self):
        return len(self.dims)

    def level(self, k):
        (h, w), o = self.dims[k], self.offsets[k]
        return self.packed[..., o:o + h * w, :].unflatten(-2, (h, w))


def build_cubemap_mipmaps(cubemap, levels=None):
    """The box-filtered mip chain of cubemap ([6,S,S,C] or [B,6,S,S,C]) as a CubeMipmaps, differentiable to the cube
    map: each face's chain is build_mipmaps' chain of that face (64 x 64 faces: seven levels, 5 x 5: one).  levels=n
    keeps at most the first n levels.  The backward is build_mipmaps': a gather in a fixed order."""
    fn = "build_cubemap_mipmaps"
    cubemap = torch.as_tensor(cubemap)
    if cubemap.dim() not in (4, 5) or cubemap.shape[-4] != 6 or min(cubemap.shape) < 1:
        raise ValueError("%s: cubemap must be a non-empty [6, S, S, C] or [B, 6, S, S, C], not %s"
                         % (fn, tuple(cubemap.shape)))
    if cubemap.shape[-3] != cubemap.shape[-2]:
        raise ValueError("%s: the faces must be square, not %s" % (fn, tuple(cubemap.shape[-3:-1])))
    if levels is not None and (not isinstance(levels, int) or levels < 1):
        raise ValueError("%s: levels must be a positive integer or None" % fn)
    S = cubemap.shape[-2]
    L = len(_mip_dims(S, S, levels))
    faces = cubemap.reshape((-1,) + cubemap.shape[-3:])  # [Cf * 6, S, S, C]: the faces as the frames of a texture
    if _FUSED_ENABLED and _gpu_f32(cubemap) and _mip_fused_texture(cubemap.shape):
        packed = _BuildMipmapsFn.apply(faces.contiguous(), L)
    else:
        packed = _build_mipmaps_ops(faces, levels).packed
    return CubeMipmaps(packed.reshape(cubemap.shape[:-3] + packed.shape[-2:]), S, L)


def _cube_mip_axis(u, T):
    """One coordinate of the tap rule, unreduced: (first tap in [-1, T - 1], weight of the second); floor has
    derivative 0."""
    x = u * T
    x = x - 0.5
    fx = torch.floor(x).detach()
    a = x - fx
    return torch.where(fx >= 0, torch.clamp(fx, max=T - 1), -1.0).to(torch.int64), a


def _cube_mip_resolve(face, i, j, T):
    """The texel that tap (i, j) of `face` resolves to at a level of T x T faces, in integers: (face', i', j', corner).
    In range: itself.  One index out of range: folded over the edge onto the neighbouring face.  Both out of range:
    `corner` is set (no texel exists; the indices returned are some valid ones)."""
    oi, oj = (i < 0) | (i >= T), (j < 0) | (j >= T)
    sc = 2 * j + 1 - T
    tc = 2 * i + 1 - T
    # the point by the inverse face table with major T
    x = torch.where(face == 0, T, torch.where(face == 1, -T, torch.where(face == 5, -sc, sc)))
    y = torch.where(face == 2, T, torch.where(face == 3, -T, -tc))
    z = torch.where(face == 0, -sc, torch.where(face == 1, sc, torch.where(face == 2, tc, torch.where(
        face == 3, -tc, torch.where(face == 4, T, -T)))))
    # the fold: the old major coordinate becomes +-(T - 1), the coordinate of magnitude T + 1 the new major +-T
    old = face >> 1
    x = torch.where(old == 0, torch.where(x < 0, 1 - T, T - 1), x)
    y = torch.where(old == 1, torch.where(y < 0, 1 - T, T - 1), y)
    z = torch.where(old == 2, torch.where(z < 0, 1 - T, T - 1), z)
    nx, ny = x.abs() > T, y.abs() > T
    face2 = torch.where(nx, (x < 0).long(), torch.where(ny, 2 + (y < 0).long(), 4 + (z < 0).long()))
    sc2 = torch.where(nx, torch.where(x < 0, z, -z), torch.where(ny, x, torch.where(z < 0, -x, x)))
    tc2 = torch.where(ny, torch.where(y < 0, -z, z), -y)
    one = oi ^ oj
    rf = torch.where(one, face2, face)
    ri = torch.clamp(torch.where(one, (tc2 + T - 1) >> 1, i), 0, T - 1)
    rj = torch.clamp(torch.where(one, (sc2 + T - 1) >> 1, j), 0, T - 1)
    return rf, ri, rj, oi & oj


def _cube_mip_level_ops(level, face, u, v, sampled, seamless):
    """The rule at one level ([6,T,T,C] or [B,6,T,T,C]) for the pixels in `sampled`: the four taps resolved, the corner
    tap the mean of the other three, then `_BilinearFn` (the value is the rule's bit for bit, the gradient to u and v
    in the kernels' difference form, and it differentiates again)."""
    T = level.shape[-2]
    j0, a = _cube_mip_axis(u, T)
    i0, b = _cube_mip_axis(v, T)
    i1, j1 = i0 + 1, j0 + 1
    if not seamless:
        i0, j0, i1, j1 = i0.clamp(min=0), j0.clamp(min=0), i1.clamp(max=T - 1), j1.clamp(max=T - 1)
    vals, corner = [], []
    for i, j in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)):
        rf, ri, rj, c = _cube_mip_resolve(face, i, j, T)
        if level.dim() == 5:
            f = torch.arange(level.shape[0], device=level.device)[:, None, None]
            vals.append(level[f, rf, ri, rj])
        else:
            vals.append(level[rf, ri, rj])
        corner.append(c[..., None])
    third = 1.0 / 3.0
    taps = []
    for n in range(4):
        p, q, r = [k for k in range(4) if k != n]
        mean = vals[p] + vals[q]
        mean = mean + vals[r]
        mean = mean * third
        taps.append(torch.where(corner[n], mean, vals[n]))
    out = _BilinearFn.apply(taps[0], taps[1], taps[2], taps[3], a[..., None], b[..., None])
    return torch.where(sampled[..., None], out, 0.0)


class _LodBlendFn(torch.autograd.Function):
    """The blend of two levels, out = s0 * (1 - f) + s1 * f, and out = s0 where f == 0 (s0, s1 [...,C], f [...,1]).
    Its gradient to f is sum_c g_c * (s1_c - s0_c) at f == 0 too: the derivative to the right, so that a lod that
    starts at an integer moves.  The backward is framework ops on the saved inputs: it differentiates again."""

    @staticmethod
    def forward(ctx, s0, s1, f):
        ctx.save_for_backward(s0, s1, f)
        return torch.where(f != 0, s0 * (1.0 - f) + s1 * f, s0)

    @staticmethod
    def backward(ctx, g):
        s0, s1, f = ctx.saved_tensors
        omf = 1.0 - f
        return g * omf, g * f, (g * (s1 - s0)).sum(-1, keepdim=True)


def _cube_mip_lod_ops(directions, valid, S, L, lod=None, lod_bias=0.0):
    """The final level of detail [...,H,W] of the rule (0 at unsampled pixels).  The automatic one is detached; an
    explicit one keeps its graph (torch.clamp passes the gradient on [0, L - 1], bounds included; a NaN gets none)."""
    if lod is None:
        d = torch.where(valid[..., None], directions.detach(), 1.0)
        m = d.abs().amax(-1, keepdim=True)
        P = d / m
        h = 0.5 * S
        q = []
        for dim in (-2, -3):
            e = _mip_difference(P, valid, dim)
            e = e * h
            qd = e[..., 0] * e[..., 0]
            t = e[..., 1] * e[..., 1]
            qd = qd + t
            t = e[..., 2] * e[..., 2]
            qd = qd + t
            q.append(qd)
        lod = _mip_lod_of_rho2(torch.fmax(q[0], q[1]), L)
    else:
        lod = lod.to(directions.dtype)
        lod = torch.where(torch.isnan(lod), 0.0, lod)
    lod = lod + lod_bias
    lod = torch.clamp(lod, 0.0, float(L - 1))
    return torch.where(valid, lod, 0.0)


def _sample_cubemap_mip_ops(chain, directions, mask=None, lod=None, lod_bias=0.0, seamless=True):
    """chain a CubeMipmaps, directions [H,W,3] or [B,H,W,3], mask and lod (directions' shape without the channels) or
    None -> (texels, valid, the final lod)."""
    S, L = chain.dims[0][0], len(chain)
    valid = torch.isfinite(directions).all(-1) & (directions != 0).any(-1)
    if mask is not None:
        valid = valid & (mask != 0)
    lod = _cube_mip_lod_ops(directions, valid, S, L, lod, lod_bias)
    k0f = torch.floor(lod).detach()
    f = (lod - k0f)[..., None]
    k0 = k0f.to(torch.int64)
    k1 = torch.clamp(k0 + 1, max=L - 1)
    above = valid & (k1 != k0)
    face, u, v = _cube_coordinates(directions, valid)
    s0 = torch.zeros(directions.shape[:-1] + (chain.packed.shape[-1],), dtype=directions.dtype,
                     device=directions.device)
    s1 = s0
    for k in range(L):  # (a level is read only by the pixels that the rule, or the lod's gradient, sends there)
        at0, at1 = valid & (k0 == k), above & (k1 == k)
        if not bool((at0 | at1).any()):
            continue
        s = _cube_mip_level_ops(chain.level(k), face, u, v, at0 | at1, seamless)
        s0 = torch.where(at0[..., None], s, s0)
        s1 = torch.where(at1[..., None], s, s1)
    s1 = torch.where(above[..., None], s1, s0)  # (the top level is its own second level: no lod gradient there)
    out = _LodBlendFn.apply(s0, s1, f)
    return torch.where(valid[..., None], out, 0.0), valid[..., None], lod.detach()


class _SampleCubemapMipFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed, directions, lod_in, mask, S, levels, lod_bias, seamless):
        Cf, _, _, C = packed.shape
        B, H, W, _ = directions.shape
        dev = directions.device
        texels = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        lod = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_cube_mip_fwd(
                packed.data_ptr(), Cf, S, C, levels, directions.data_ptr(), _ptr(mask), _ptr(lod_in), lod_bias, B, H,
                W, seamless, texels.data_ptr(), valid.data_ptr(), lod.data_ptr(), _stream(dev)))
        ctx.save_for_backward(packed, directions, lod_in, mask, lod)
        ctx.args = (S, levels, lod_bias, seamless)
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid, lod)
        ctx.set_materialize_grads(False)  # (as sample_texture_mip: no zero-filled "gradient" of valid or the lod)
        return texels, valid, lod

    @staticmethod
    def backward(ctx, grad_texels, _grad_valid, _grad_lod):
        _no_double_backward("sample_cubemap_mip")
        if grad_texels is None:
            return (None,) * 8
        packed, directions, lod_in, mask, lod = ctx.saved_tensors
        S, levels, lod_bias, seamless = ctx.args
        Cf, _, _, C = packed.shape
        B, H, W, _ = directions.shape
        dev = directions.device
        grad_texels = grad_texels.contiguous()
        # (NULL for the gradient nobody needs: the kernel then skips it; grad_packed is zero-filled by the call)
        grad_packed = torch.empty_like(packed) if ctx.needs_input_grad[0] else None
        grad_directions = torch.empty_like(directions) if ctx.needs_input_grad[1] else None
        grad_lod = torch.empty_like(lod_in) if lod_in is not None and ctx.needs_input_grad[2] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_texture_sample_cube_mip_bwd(
                packed.data_ptr(), Cf, S, C, levels, directions.data_ptr(), _ptr(mask), _ptr(lod_in), lod_bias,
                lod.data_ptr(), B, H, W, seamless, grad_texels.data_ptr(), _ptr(grad_packed), _ptr(grad_directions),
                _ptr(grad_lod), _stream(dev)))
        return (grad_packed, grad_directions, grad_lod) + (None,) * 5


def _sample_cubemap_mip(chain, directions, mask=None, lod=None, lod_bias=0.0, seamless=True):
    """sample_cubemap_mip with the pixels' final lod as a third result (the buffer the fused backward reads)."""
    fn = "sample_cubemap_mip"
    if not isinstance(chain, CubeMipmaps):
        chain = build_cubemap_mipmaps(chain)
    packed = chain.packed
    directions = torch.as_tensor(directions, dtype=packed.dtype, device=packed.device)
    if directions.dim() not in (3, 4) or directions.shape[-1] != 3:
        raise ValueError("%s: directions must be [H, W, 3] or [B, H, W, 3]" % fn)
    if packed.dim() == 4 and (directions.dim() != 4 or packed.shape[0] != directions.shape[0]):
        raise ValueError("%s: a per-frame chain of shape %s for directions of shape %s"
                         % (fn, tuple(packed.shape), tuple(directions.shape)))
    mask = _checked_mask(fn, mask, directions, "directions")
    if lod is not None:
        lod = torch.as_tensor(lod, device=directions.device)
        if lod.shape != directions.shape[:-1] or not lod.is_floating_point():
            raise ValueError("%s: lod must be a float tensor of shape %s, not %s"
                             % (fn, tuple(directions.shape[:-1]), tuple(lod.shape)))
    if isinstance(lod_bias, torch.Tensor) or not float("-inf") < float(lod_bias) < float("inf"):
        raise ValueError("%s: lod_bias must be a finite number" % fn)
    lod_bias = float(lod_bias)
    S, L = chain.dims[0][0], len(chain)
    if (_FUSED_ENABLED and _gpu_f32(packed, directions) and _mip_fused_texture((S, S, packed.shape[-1])) and
            L <= _lib.MAX_MIP_LEVELS and 1 <= min(directions.shape[-3:-1]) and
            max(directions.shape[-3:-1]) <= _lib.MAX_DIM and (mask is None or mask.device == directions.device)):
        (pb, _), (db, added) = _batched(packed, 4), _batched(directions)
        lb = None if lod is None else lod.to(torch.float32).contiguous().reshape(db.shape[:-1])
        return _unbatched(_SampleCubemapMipFn.apply(pb, db, lb, _kernel_mask(mask, db), S, L, lod_bias,
                                                    1 if seamless else 0), added)
    return _sample_cubemap_mip_ops(chain, directions, mask, lod, lod_bias, seamless)


def sample_cubemap_mip(chain, directions, mask=None, lod=None, lod_bias=0.0, seamless=True):
    """Trilinear lookup of a cube map's mip chain (a CubeMipmaps, or a plain cube map [6,S,S,C] / [B,6,S,S,C] whose
    chain is built inside the call) at directions, with sample_cubemap's conventions for the faces, the directions,
    the mask, the sampled pixels and the two results (texels, valid).

    The level of detail is lod ([H,W] or [B,H,W], float; a NaN counts as 0) -- a roughness map scaled to levels, say --
    or, with lod=None, taken per pixel from the differences of the point P = direction / |major component| on the
    unit cube to the sampled neighbours (the next pixel in x and in y where there is one, else the previous one, else
    0), scaled by S / 2 to texels: rho2 = max(|d_x|^2, |d_y|^2) and sample_texture_mip's piecewise-linear log2.  P is
    continuous across the face seams, so the automatic lod is too.  lod_bias is added, the sum clamped to
    [0, levels - 1], and the result is level floor(lod) blended with the next level by the fractional part (an integer
    lod reads one level only).

    With seamless=True every level is filtered across the face seams, in the manner of GL_TEXTURE_CUBE_MAP_SEAMLESS: a
    tap past a face's edge is the texel of the neighbouring face next to it, and the one tap past a cube corner, where
    no texel exists, is the mean of the other three.  seamless=False clamps to the face's edge at every level, which is
    sample_cubemap's rule.

    Gradients reach the chain (and through build_cubemap_mipmaps the cube map), the directions (the blend of the two
    levels' sample_cubemap gradients, taken on the resolved taps) and an explicit lod: sum_c g_c * (s_k1 - s_k0), by
    torch.clamp's rule zero outside [0, levels - 1], and at an integer lod the derivative to the right, so that a
    roughness map initialised at 0 is not stuck there.  The automatic lod carries no gradient.  On the GPU the
    directions' and the lod's gradients are bit-identical from run to run; the chain's is summed with float atomics."""
    return _sample_cubemap_mip(chain, directions, mask, lod, lod_bias, seamless)[:2]


# ---- shadow-map lookup

def _sample_shadow_ops(depth_map, positions, light_matrix, bias=0.0, softness=0.0, mask=None):
    """depth_map [Sh,Sw,1] or [B,Sh,Sw,1], positions [H,W,3] or [B,H,W,3], light_matrix [4,4] or [B,4,4], mask
    (positions' shape without the channels) or None.  The rule of dirt_amd/csrc/shadow_kernels.h, each line one
    operation in the operands' dtype."""
    dt, dev = positions.dtype, positions.device
    valid = torch.isfinite(positions).all(-1) if mask is None else mask != 0
    M = light_matrix if light_matrix.dim() == 2 else light_matrix[:, None, None]

    def clip(p):
        c = ((p[..., 0:1] * M[..., 0, :] + p[..., 1:2] * M[..., 1, :]) + p[..., 2:3] * M[..., 2, :]) + M[..., 3, :]
        return c.unbind(-1)

    def coordinates(cx, cy, cw):
        iw = 1.0 / cw
        return (cx * iw) * 0.5 + 0.5, 0.5 - (cy * iw) * 0.5

    # which pixels are inside the light's frustum is decided on the raw positions, without a graph; the
    # differentiable pass then starts from operands made harmless wherever a pixel is not inside (an inside pixel
    # has finite positions and cw > 0, and its values are the first pass's), so that no 0 * inf reaches a gradient
    with torch.no_grad():
        cx, cy, _, cw = clip(positions)
        u, v = coordinates(cx, cy, cw)
        inside = valid & (cw > 0) & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    cx, cy, cz, cw = clip(torch.where(inside[..., None], positions, 0.0))
    u, v = coordinates(torch.where(inside, cx, 0.0), torch.where(inside, cy, 0.0), torch.where(inside, cw, 1.0))
    Sh, Sw = depth_map.shape[-3], depth_map.shape[-2]
    j0, j1, a = _texture_axis(u, Sw, "clamp")
    i0, i1, b = _texture_axis(v, Sh, "clamp")
    d = depth_map[..., 0]
    if d.dim() == 3:
        f = torch.arange(d.shape[0], device=d.device)[:, None, None]
        taps = d[f, i0, j0], d[f, i0, j1], d[f, i1, j0], d[f, i1, j1]
    else:
        taps = d[i0, j0], d[i0, j1], d[i1, j0], d[i1, j1]
    zc = cz - torch.full((), bias, dtype=dt, device=dev)
    if softness > 0:
        inv = torch.ones((), dtype=dt, device=dev) / torch.full((), softness, dtype=dt, device=dev)
        s00, s01, s10, s11 = (torch.clamp((t - zc) * inv + 1.0, 0.0, 1.0) for t in taps)
    else:
        s00, s01, s10, s11 = ((t >= zc).to(dt) for t in taps)
    oma, omb = 1.0 - a, 1.0 - b
    top = s00 * oma + s01 * a
    bot = s10 * oma + s11 * a
    out = top * omb + bot * b
    lit = valid.to(dt)  # (a sampled pixel outside the frustum, or behind the light, is lit)
    return torch.where(inside, out, lit)[..., None], valid[..., None]


class _SampleShadowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_map, positions, matrix, mask, bias, softness):
        Sf, Sh, Sw, _ = depth_map.shape
        B, H, W, _ = positions.shape
        dev = positions.device
        visibility = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev)
        valid = torch.empty((B, H, W, 1), dtype=torch.uint8, device=dev)
        ctx.args = (1 if matrix.dim() == 3 else 0, bias, softness)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dirt_shadow_sample_fwd(
                depth_map.data_ptr(), Sf, Sh, Sw, positions.data_ptr(), _ptr(mask), B, H, W, ctx.args[0],
                matrix.data_ptr(), bias, softness, visibility.data_ptr(), valid.data_ptr(), _stream(dev)))
        ctx.save_for_backward(depth_map, positions, matrix, mask)
        valid = valid.view(torch.bool)  # (the kernel writes 0 / 1)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # (as the shade: no zero-filled "gradient" of valid)
        return visibility, valid

    @staticmethod
    def backward(ctx, grad_visibility, _grad_valid):
        _no_double_backward("sample_shadow")
        if grad_visibility is None:
            return (None,) * 6
        depth_map, positions, matrix, mask = ctx.saved_tensors
        matrix_pf, bias, softness = ctx.args
        Sf, Sh, Sw, _ = depth_map.shape
        B, H, W, _ = positions.shape
        dev = positions.device
        grad_visibility = grad_visibility.contiguous()
        # (NULL for the gradients nobody needs: the kernel then skips them, and without the matrix's the partial
        # sums and the second launch as well; grad_depth is zero-filled by the call)
        grads = [torch.empty_like(t) if need else None
                 for t, need in zip((depth_map, positions, matrix), ctx.needs_input_grad[:3])]
        lib = _lib.load()
        workspace, size = None, _lib._SZ(0)
        if grads[2] is not None:
            _lib.check(lib.dirt_shadow_sample_workspace(B, H, W, ctypes.byref(size)))
            workspace = torch.empty((max(size.value, 4),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.dirt_shadow_sample_bwd(
                depth_map.data_ptr(), Sf, Sh, Sw, positions.data_ptr(), _ptr(mask), B, H, W, matrix_pf,
                matrix.data_ptr(), bias, softness, grad_visibility.data_ptr(), _ptr(grads[0]), _ptr(grads[1]),
                _ptr(grads[2]), _ptr(workspace), size.value, _stream(dev)))
        return tuple(grads) + (None, None, None)


def _shadow_number(fn, x, name):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 <= float(x) < float("inf"):
        raise ValueError("%s: %s must be a finite Python number >= 0" % (fn, name))
    return float(x)


def sample_shadow(depth_map, positions, light_matrix, bias=0.0, softness=0.0, mask=None):
    """The visibility of a light at the pixels of a world-position G-buffer, from the light's shadow map.

    depth_map ([Sh,Sw,1]: shared by every frame, its gradient sums over them; or [B,Sh,Sw,1]: one per frame) is what
    `rasterise(..., channels=1)` returns for a render from the light with vertices = [Vw,1] @ light_matrix,
    vertex_colors = that[:, 2:3] and background = +inf: the light's clip-space z before the divide (affine in the
    world position under orthographic and perspective matrices alike, so the rasteriser interpolates it exactly),
    +inf where nothing was drawn.  positions ([H,W,3] or [B,H,W,3]) is the world-position G-buffer over its -inf
    background; the op does not dilate (pass `dilate(positions)` for the silhouette ring).  light_matrix ([4,4] or
    [B,4,4]) is in dirt_amd.matrices' row-vector convention, clip = [p,1] @ M, and may need a gradient.  bias and
    softness are Python numbers >= 0 in clip-z units.  A pixel is sampled where mask ([H,W] or [B,H,W]) is nonzero;
    mask=None samples the pixels whose three position channels are finite.

    A sampled pixel behind the light (cw <= 0) or outside its frustum (u = cx / cw / 2 + 1/2, v = 1/2 - cy / cw / 2
    not both in [0,1]) is lit: visibility 1, no gradient.  Inside, the four taps of sample_texture's clamp rule at
    (u, v) are compared with zc = cz - bias, s = d >= zc (softness == 0: 2 x 2 percentage-closer filtering) or
    s = clamp((d - zc) / softness + 1, 0, 1) (a tap is fully lit at d + bias >= cz, fully shadowed at d + bias <=
    cz - softness), and blended bilinearly.

    Returns (visibility, valid): visibility [...,H,W,1] in [0,1], exactly 0 at unsampled pixels; valid [...,H,W,1]
    bool marks the sampled pixels and carries no gradient.  Gradients reach the depth map (through the ramp, so only
    at softness > 0; never at a non-finite texel), the positions and the light matrix (through the ramp into cz and
    through the bilinear weights into cx, cy and cw).  On the GPU the positions' and the matrix's gradients are
    bit-identical from run to run (the matrix's is summed in a fixed order, without atomics); the depth map's is
    summed with float atomics and may differ in the last bits.

    Use it with one shade_lights call per shadowed light (N = 1, ambient_color=None) multiplied by that light's
    visibility, plus one ambient call."""
    fn = "sample_shadow"
    positions = torch.as_tensor(positions)
    dt, dev = positions.dtype, positions.device
    depth_map = torch.as_tensor(depth_map, dtype=dt, device=dev)
    if not isinstance(light_matrix, torch.Tensor):
        light_matrix = torch.as_tensor(light_matrix, dtype=dt, device=dev)
    if positions.dim() not in (3, 4) or positions.shape[-1] != 3:
        raise ValueError("%s: positions must be [H, W, 3] or [B, H, W, 3]" % fn)
    if depth_map.dim() not in (3, 4) or depth_map.shape[-1] != 1 or min(depth_map.shape[-3:]) < 1:
        raise ValueError("%s: depth_map must be a non-empty [Sh, Sw, 1] or [B, Sh, Sw, 1]" % fn)
    if depth_map.dim() == 4 and (positions.dim() != 4 or depth_map.shape[0] != positions.shape[0]):
        raise ValueError("%s: a per-frame depth_map of shape %s for positions of shape %s"
                         % (fn, tuple(depth_map.shape), tuple(positions.shape)))
    frames = positions.shape[0] if positions.dim() == 4 else None
    if tuple(light_matrix.shape) not in ((4, 4), (frames, 4, 4)):
        raise ValueError("%s: light_matrix must be [4, 4] or [B, 4, 4]" % fn)
    bias, softness = _shadow_number(fn, bias, "bias"), _shadow_number(fn, softness, "softness")
    mask = _checked_mask(fn, mask, positions, "positions")
    if (_FUSED_ENABLED and _gpu_f32(positions, depth_map, light_matrix) and
            max(depth_map.shape[-3], depth_map.shape[-2]) <= _lib.MAX_DIM and
            1 <= min(positions.shape[-3:-1]) and max(positions.shape[-3:-1]) <= _lib.MAX_DIM and
            (mask is None or mask.device == dev)):
        (db, _), (pb, added) = _batched(depth_map), _batched(positions)
        return _unbatched(_SampleShadowFn.apply(db, pb, light_matrix.contiguous(), _kernel_mask(mask, pb), bias,
                                                softness), added)
    if light_matrix.dtype != dt or light_matrix.device != dev:
        light_matrix = light_matrix.to(device=dev, dtype=dt)
    return _sample_shadow_ops(depth_map, positions, light_matrix, bias, softness, mask)
