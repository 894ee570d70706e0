"""The pixel-space stage of deferred shading: silhouette dilation and G-buffer lighting.

The reference's sample (samples/deferred.py:85-115) dilates the position and normal G-buffers by a 3x3 max where the
background shows, then adds ambient, diffuse_directional and specular_directional per pixel.  Its blend
`x * (1 - mask) + dilated * mask` turns every background pixel into NaN (-inf * 0); here the blend is a select, pixels
the dilation does not reach are left out of the shading (exactly 0, `valid` False) and no NaN reaches a gradient.

  dilate(x, mask=None)     [H,W,C] or [B,H,W,C]: the 3x3 max where mask is set (default: any channel is +-inf)
  shade(positions, colors, normals, ...) -> (pixels, valid)
  sample_texture(texture, uv, mask=None, wrap="clamp") -> (texels, valid): bilinear texture lookup at a uv G-buffer

On the GPU both run as one fused HIP launch forward and one backward (dirt_amd/csrc/deferred_kernels.h, C ABI
dirt_dilate_* / dirt_deferred_shade_*) when their operands are float32 tensors on one GPU and the light parameters
are [3] float32 tensors on it that need no gradient, with a Python-number shininess.  Anything else -- CPU tensors,
other dtypes, gradients with respect to the light, a tensor-valued shininess -- runs the framework-op statement below
(`_dilate_ops`, `_shade_ops`).  The max follows the framework's CPU max_pool2d: the first maximum wins ties, a NaN in
the window gives NaN.  The fused backwards are gathers in a fixed order: their gradients are bit-identical from run
to run.  They are kernels, not differentiable graphs: `create_graph=True` through them raises RuntimeError;
DIRT_FUSED_DEFERRED=0 routes every call to the framework ops (double backward supported).

sample_texture is the step between the two: UV -> texel, with gradients to the texture and through the uv into the
geometry (dirt_amd/csrc/texture_kernels.h, C ABI dirt_texture_sample_*; the statement is `_sample_texture_ops`).  Its
uv gradient is a gather in a fixed order too; its texture gradient is a scatter-add summed with float atomics (per
screen tile in an LDS patch first), so it may differ in the last bits from run to run, as vertex_normals' does.
"""
import os

import torch
import torch.nn.functional as Fn

from . import _lib
from .lighting import _diffuse_directional_ops, _gpu_f32, _light_param, _specular_directional_ops

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
    if mask is not None:
        mask = torch.as_tensor(mask, device=x.device)
        if mask.shape != x.shape[:-1]:
            raise ValueError("dilate: mask of shape %s for x of shape %s" % (tuple(mask.shape), tuple(x.shape)))
    if (_FUSED_ENABLED and _gpu_f32(x) and 1 <= x.shape[-1] <= _lib.MAX_CHANNELS and
            (mask is None or mask.device == x.device)):
        xb = x.contiguous() if x.dim() == 4 else x.contiguous()[None]
        mb = None
        if mask is not None:
            mb = (mask if mask.dtype == torch.bool else mask != 0).contiguous().view(torch.uint8)
        out = _DilateFn.apply(xb, mb)
        return out if x.dim() == 4 else out[0]
    return _dilate_ops(x, mask)


# ---- shade

def _shade_ops(positions, colors, normals, ambient_color, light_direction, diffuse_color, specular_color,
               camera_position, shininess, double_sided=False):
    dev, dt = positions.device, positions.dtype
    bg = torch.isinf(positions).any(-1)
    pos_d = _dilate_ops(positions, bg)
    nrm_d = _dilate_ops(normals, bg)
    valid = torch.isfinite(pos_d).all(-1, keepdim=True) & torch.isfinite(nrm_d).all(-1, keepdim=True)
    pos_s, nrm_s, col_s = (torch.where(valid, x, 0.0) for x in (pos_d, nrm_d, colors))
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
    positions = torch.as_tensor(positions)
    dev, dt = positions.device, positions.dtype
    colors, normals = (torch.as_tensor(x, dtype=dt, device=dev) for x in (colors, normals))
    if positions.dim() not in (3, 4) or positions.shape[-1] != 3 or colors.shape != positions.shape or \
            normals.shape != positions.shape:
        raise ValueError("shade: positions, colors, normals must share one shape [H, W, 3] or [B, H, W, 3]")
    if _FUSED_ENABLED and _gpu_f32(positions, colors, normals) and isinstance(shininess, (int, float)):
        ps = [_light_param(x, positions) for x in (ambient_color, light_direction, diffuse_color, specular_color,
                                                   camera_position)]
        if all(p is not None for p in ps):
            ops = [x.contiguous() if x.dim() == 4 else x.contiguous()[None] for x in (positions, colors, normals)]
            pixels, valid = _ShadeFn.apply(*ops, *ps, float(shininess), 1 if double_sided else 0)
            return (pixels, valid) if positions.dim() == 4 else (pixels[0], valid[0])
    return _shade_ops(positions, colors, normals, ambient_color, light_direction, diffuse_color, specular_color,
                      camera_position, shininess, double_sided)


# ---- texture sampling

_WRAPS = {"clamp": _lib.TEXTURE_CLAMP, "repeat": _lib.TEXTURE_REPEAT}


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


def _sample_texture_ops(texture, uv, mask=None, wrap="clamp"):
    """texture [Th,Tw,C] or [B,Th,Tw,C], uv [H,W,2] or [B,H,W,2], mask (uv's shape without the channels) or None."""
    Th, Tw = texture.shape[-3], texture.shape[-2]
    valid = torch.isfinite(uv).all(-1) if mask is None else mask != 0
    uvs = torch.where(valid[..., None], uv, 0.0)  # (no index is ever formed from an unsampled pixel's uv)
    j0, j1, a = _texture_axis(uvs[..., 0], Tw, wrap)
    i0, i1, b = _texture_axis(uvs[..., 1], Th, wrap)
    if texture.dim() == 4:
        f = torch.arange(texture.shape[0], device=texture.device)[:, None, None]
        t00, t01, t10, t11 = texture[f, i0, j0], texture[f, i0, j1], texture[f, i1, j0], texture[f, i1, j1]
    else:
        t00, t01, t10, t11 = texture[i0, j0], texture[i0, j1], texture[i1, j0], texture[i1, j1]
    a, b = a[..., None], b[..., None]
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
    if mask is not None:
        mask = torch.as_tensor(mask, device=uv.device)
        if mask.shape != uv.shape[:-1]:
            raise ValueError("sample_texture: mask of shape %s for uv of shape %s"
                             % (tuple(mask.shape), tuple(uv.shape)))
    if (_FUSED_ENABLED and _gpu_f32(texture, uv) and 1 <= texture.shape[-1] <= _lib.MAX_CHANNELS and
            max(texture.shape[-3], texture.shape[-2]) <= _lib.MAX_DIM and
            1 <= min(uv.shape[-3:-1]) and max(uv.shape[-3:-1]) <= _lib.MAX_DIM and
            (mask is None or mask.device == uv.device)):
        tb = texture.contiguous() if texture.dim() == 4 else texture.contiguous()[None]
        ub = uv.contiguous() if uv.dim() == 4 else uv.contiguous()[None]
        mb = None
        if mask is not None:
            mb = (mask if mask.dtype == torch.bool else mask != 0).contiguous().view(torch.uint8).reshape(ub.shape[:-1])
        texels, valid = _SampleTextureFn.apply(tb, ub, mb, _WRAPS[wrap])
        return (texels, valid) if uv.dim() == 4 else (texels[0], valid[0])
    return _sample_texture_ops(texture, uv, mask, wrap)
