"""The film's maths for the derivative passes of ``integrators``: the reconstruction filter's window around a sample, the
adjoint and the forward mode of splat + weight division (ImageBlock::put + film.develop), the fixed-point weight channel.
The gaussian and the box window are each written ONCE here; every function below takes its weights from them."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib


def _box_window(film_pos: torch.Tensor, H: int, W: int):
    """The pixel under every sample, (X, Y) (n) each, and whether it is on the film."""
    X, Y = torch.floor(film_pos[:, 0]).long(), torch.floor(film_pos[:, 1]).long()
    return X, Y, (X >= 0) & (Y >= 0) & (X < W) & (Y < H)


def _gaussian_window(film_pos: torch.Tensor, H: int, W: int, derivatives: bool = False):
    """The 5 x 5 window of the gaussian reconstruction filter (stddev 0.5, radius 2, src/rfilters/gaussian.cpp) around every
    sample: pixel columns ``xs`` and rows ``ys`` (n,5) each, not clamped, and the separable weights ``wx``, ``wy`` (n,5), zero
    off the film.  The weight of pixel (ys[i,a], xs[i,b]) is wy[i,a] wx[i,b].  ``derivatives``: ``dwx``, ``dwy`` (n,5) too, the
    weights' derivatives in the sample's film position."""
    px, py = film_pos[:, 0], film_pos[:, 1]
    X, Y = torch.floor(px).long(), torch.floor(py).long()
    radius, alpha = 2.0, -1.0 / (2.0 * 0.5 * 0.5)
    bias = math.exp(alpha * radius * radius)
    off = torch.arange(-2, 3, device=film_pos.device)
    xs, ys = X[:, None] + off[None, :], Y[:, None] + off[None, :]             # (n,5)

    def axis(d_, inside):                                  # d_ = pixel centre - pos
        e = torch.exp(alpha * d_ * d_)
        w = torch.where(d_.abs() <= radius, (e - bias).clamp_min(0), torch.zeros_like(d_)) * inside
        # d w / d pos where the weight is live: inside the radius, on the film and above the bias, i.e. w > 0
        return w, torch.where(w > 0, -2.0 * alpha * d_ * e, torch.zeros_like(d_)) if derivatives else None
    wx, dwx = axis((xs.float() + 0.5) - px[:, None], (xs >= 0) & (xs < W))
    wy, dwy = axis((ys.float() + 0.5) - py[:, None], (ys >= 0) & (ys < H))
    return (xs, ys, wx, wy, dwx, dwy) if derivatives else (xs, ys, wx, wy)


def film_adjoint(film_pos: torch.Tensor, grad_img: torch.Tensor, weight_img: torch.Tensor, rfilter: int) -> torch.Tensor:
    """Adjoint of ImageBlock::put + film.develop (``epsm_film_splat`` / ``epsm_film_develop``) w.r.t. the radiance of
    every sample: image[p] = sum_i w_ip L_i / W_p, so dL_i = sum_p grad[p] w_ip / W_p -- the box filter touches the
    pixel under the sample, the gaussian (stddev 0.5, radius 2, src/rfilters/gaussian.cpp) its 5x5 window.
    ``film_pos (n,2)``, ``grad_img (H,W,3)``, ``weight_img (H,W)`` = W_p of the primal pass; returns ``(n,3)``."""
    H, W = weight_img.shape
    g = grad_img[..., :3] / weight_img.clamp_min(1e-30)[..., None]
    g = torch.where((weight_img > 0)[..., None], g, torch.zeros_like(g))
    if rfilter == 0:                                      # EPSM_RFILTER_BOX
        X, Y, ok = _box_window(film_pos, H, W)
        return g[Y.clamp(0, H - 1), X.clamp(0, W - 1)] * ok[:, None]
    xs, ys, wx, wy = _gaussian_window(film_pos, H, W)
    gw = g[ys.clamp(0, H - 1)[:, :, None], xs.clamp(0, W - 1)[:, None, :]]      # (n,5,5,3)
    return (gw * (wy[:, :, None] * wx[:, None, :])[..., None]).sum(dim=(1, 2))


_WEIGHT_ONE = float(1 << 40)


def film_weight_counts(counts: torch.Tensor, film_pos: torch.Tensor, rfilter: int) -> None:
    """The film's weight channel W_p = sum_i w_ip of a tile's samples in FIXED POINT: adds round(w_ip 2^40) to ``counts`` (H,W)
    int64.  Integer addition is associative, so the sums are the same bits in whatever order the adds land -- unlike the float
    atomics of ``epsm_film_splat``, whose weight channel differs in its last bits from call to call.  The roughness adjoint is
    summed without atomics so that a call repeats bit for bit; the adjoint radiance it is fed divides by W_p, so W_p must repeat
    too.  (2^-40 per sample is far below float32's resolution; 2^23 samples of weight 1 fit a pixel.)"""
    H, W = counts.shape
    flat = counts.view(-1)
    if rfilter == 0:                                      # EPSM_RFILTER_BOX
        X, Y, ok = _box_window(film_pos, H, W)
        flat.index_add_(0, Y.clamp(0, H - 1) * W + X.clamp(0, W - 1), ok.long() << 40)
        return
    xs, ys, wx, wy = _gaussian_window(film_pos, H, W)
    w = torch.round((wy[:, :, None] * wx[:, None, :]).double() * _WEIGHT_ONE).long()              # (n,5,5)
    idx = ys.clamp(0, H - 1)[:, :, None] * W + xs.clamp(0, W - 1)[:, None, :]
    flat.index_add_(0, idx.reshape(-1), w.reshape(-1))


def film_adjoint_reparam(film_pos: torch.Tensor, radiance: torch.Tensor, grad_img: torch.Tensor, accum: torch.Tensor):
    """Adjoint of the gaussian splat + weight division w.r.t. a sample's radiance, its FILM POSITION and the determinant
    of the reparameterisation that multiplies both its value and its weight (common.py:880-920):
        image[p] = sum_i w_ip L_i det_i / sum_i w_ip det_i,   w_ip = f(p - pos_i)
    ``accum (H,W,4)``: the film [r,g,b,w] of the primal pass.  Returns ``dL (n,3)`` and ``adj (n,3)`` =
    [d loss / d pos.x, d loss / d pos.y, d loss / d det] at det = 1.
    On the GPU: ONE kernel (``epsm_film_adjoint_reparam``, include/epsm_trace.h); the torch form below is what it is checked
    against (tests/test_gpu_reparam.py) and what the host build of the tracer runs with."""
    if film_pos.is_cuda:
        n = int(film_pos.shape[0])
        fp, rad = film_pos.detach().float().contiguous(), radiance.detach().float().contiguous()
        g, acc = grad_img.detach().float().contiguous(), accum.detach().float().contiguous()
        dL = torch.empty((n, 3), device=film_pos.device, dtype=torch.float32)
        adj = torch.empty((n, 3), device=film_pos.device, dtype=torch.float32)
        stream = _lib.stream(film_pos.device)
        _lib.check(_lib.lib().epsm_film_adjoint_reparam(n, fp.data_ptr(), rad.data_ptr(), g.data_ptr(), int(g.shape[-1]), acc.data_ptr(),
                                                         int(acc.shape[1]), int(acc.shape[0]), dL.data_ptr(), adj.data_ptr(),
                                                         C.c_void_p(stream)), "epsm_film_adjoint_reparam")
        return dL, adj
    return film_adjoint_reparam_torch(film_pos, radiance, grad_img, accum)


def film_adjoint_reparam_torch(film_pos: torch.Tensor, radiance: torch.Tensor, grad_img: torch.Tensor, accum: torch.Tensor):
    """``film_adjoint_reparam`` as dense torch operations (the checker of the HIP kernel; the CPU path of the host harness)."""
    H, W = accum.shape[:2]
    Wp = accum[..., 3]
    ok = (Wp > 0)[..., None]
    inv = torch.where(ok, 1.0 / Wp.clamp_min(1e-30)[..., None], torch.zeros_like(accum[..., :1]))
    g = grad_img[..., :3] * inv                                     # grad / W_p
    gi = (g * (accum[..., :3] * inv)).sum(-1)                       # (grad . image) / W_p
    xs, ys, wx, wy, dwx, dwy = _gaussian_window(film_pos, H, W, derivatives=True)
    yi, xi = ys.clamp(0, H - 1)[:, :, None], xs.clamp(0, W - 1)[:, None, :]
    gw = g[yi, xi]                                                   # (n,5,5,3)
    A = (gw * radiance[:, None, None, :]).sum(-1) - gi[yi, xi]       # (n,5,5): grad_p . (L_i - image_p) / W_p
    w2 = wy[:, :, None] * wx[:, None, :]
    dL = (gw * w2[..., None]).sum(dim=(1, 2))
    adj = torch.stack([(A * (wy[:, :, None] * dwx[:, None, :])).sum(dim=(1, 2)),
                       (A * (dwy[:, :, None] * wx[:, None, :])).sum(dim=(1, 2)), (A * w2).sum(dim=(1, 2))], dim=1)
    return dL.contiguous(), adj.contiguous()


def film_splat_tangent(d_accum: torch.Tensor, film_pos: torch.Tensor, radiance: torch.Tensor, d_radiance: torch.Tensor,
                       d_film: Optional[torch.Tensor], rfilter: int) -> None:
    """Forward mode of splat + weight division, the transpose of ``film_adjoint_reparam`` (and, with ``d_film`` None, of
    ``film_adjoint``): ACCUMULATES into ``d_accum (H,W,4)``, per pixel p,
        dA_p += (grad f(p - pos_i) . d pos_i + f d det_i) L_i + f d L_i,    dW_p += grad f . d pos_i + f d det_i
    for the samples' film positions (n,2), radiance (n,3) and tangents ``d_radiance (n,3)``, ``d_film (n,3)`` = [d pos.x, d pos.y,
    d det] (None: the samples do not move).  ``develop_tangent`` turns the film and this into the image's tangent.
    On the GPU: ONE kernel (``epsm_film_splat_tangent``, include/epsm_trace.h); the torch form is its checker and the CPU path."""
    if film_pos.is_cuda:
        n = int(film_pos.shape[0])
        fp, rad, drad = film_pos.detach().float().contiguous(), radiance.detach().float().contiguous(), d_radiance.detach().float().contiguous()
        dfilm = None if d_film is None else d_film.detach().float().contiguous()
        assert d_accum.is_contiguous() and d_accum.dtype == torch.float32
        _lib.check(_lib.lib().epsm_film_splat_tangent(n, fp.data_ptr(), rad.data_ptr(), drad.data_ptr(),
                                                       None if dfilm is None else dfilm.data_ptr(), int(d_accum.shape[1]),
                                                       int(d_accum.shape[0]), int(rfilter), d_accum.data_ptr(),
                                                       C.c_void_p(_lib.stream(film_pos.device))), "epsm_film_splat_tangent")
        return
    d_accum += film_splat_tangent_torch(film_pos, radiance, d_radiance, d_film, d_accum.shape[0], d_accum.shape[1], rfilter)


def film_splat_tangent_torch(film_pos: torch.Tensor, radiance: torch.Tensor, d_radiance: torch.Tensor, d_film: Optional[torch.Tensor],
                             H: int, W: int, rfilter: int) -> torch.Tensor:
    """``film_splat_tangent`` as dense torch operations: returns the (H,W,4) tangent film of the samples."""
    out = torch.zeros((H * W, 4), device=film_pos.device, dtype=torch.float32)
    if rfilter == 0:                                      # EPSM_RFILTER_BOX: the weight does not move with the sample
        if d_film is not None:
            raise ValueError("film_splat_tangent: a box filter has no derivative in the film position")
        X, Y, ok = _box_window(film_pos, H, W)
        out[:, :3].index_add_(0, (Y * W + X)[ok], d_radiance[ok].float())
        return out.view(H, W, 4)
    xs, ys, wx, wy, dwx, dwy = _gaussian_window(film_pos, H, W, derivatives=True)
    w2 = wy[:, :, None] * wx[:, None, :]                                     # (n,5,5)
    if d_film is None:
        dw = torch.zeros_like(w2)
    else:
        fx, fy, fd = d_film[:, 0, None, None], d_film[:, 1, None, None], d_film[:, 2, None, None]
        dw = wy[:, :, None] * dwx[:, None, :] * fx + dwy[:, :, None] * wx[:, None, :] * fy + w2 * fd
    rgb = dw[..., None] * radiance[:, None, None, :] + w2[..., None] * d_radiance[:, None, None, :]
    inside = ((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :]
    idx = (ys.clamp(0, H - 1)[:, :, None] * W + xs.clamp(0, W - 1)[:, None, :])[inside]
    out.index_add_(0, idx, torch.cat([rgb, dw[..., None]], dim=-1)[inside])
    return out.view(H, W, 4)


def develop_tangent(accum: torch.Tensor, d_accum: torch.Tensor) -> torch.Tensor:
    """The tangent of the developed image A / W: (dA - image dW) / W, zero where the primal film has no weight."""
    Wp = accum[..., 3:4]
    inv = torch.where(Wp > 0, 1.0 / Wp.clamp_min(1e-30), torch.zeros_like(Wp))
    return (d_accum[..., :3] - accum[..., :3] * inv * d_accum[..., 3:4]) * inv
