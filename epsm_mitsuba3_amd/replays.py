"""The replays of the colour adjoint, one record each: ``epsm_trace_paths_<stem>_{backward,forward}`` of include/epsm_trace.h
replay the paths of ``epsm_trace_paths_color`` and differentiate one kind of parameter along them.  Everything the driver side
knows kind by kind stands here once: ``_lib.declare_tracer`` takes the prototypes from it, ``Scene.replay_backward`` /
``replay_forward`` the call, ``PRBIntegrator`` what is attached, the buffers and where they end up in a ``ParamGrads``.

A ``Replay`` is one pair of entry points; a ``Section`` is the part of a ``ParamGrads`` it differentiates.  The two texel kinds
point at ONE section: one flat buffer, one all-reduce and one deposit per call.  The order of ``REPLAYS`` is the order in which a
tile's replays are called and their d radiance is added, and the order of the sections' all-reduces: float addition order
decides bits, so it is part of the contract.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from .params import tex_numel, tex_shape, tex_view


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device, torch.float32)


# -- sections: check(scene, params, what) raises unless ``params`` ("gradient buffer" / "tangent") is laid out for what is
#    attached; zeros -> (the one tensor a call all-reduces, the buffer its replays accumulate into); tangent -> the buffer the
#    forward replays read; deposit adds the all-reduced buffer to ``params`` -------------------------------------------------
def _texel_check(scene, params, what):
    if params.tex_shapes != [tex_shape(t) for t in scene.texture_shapes()]:
        raise ValueError(f"texture slots are attached: the {what} must come from Scene.param_grads() after attach_texture")


def _texel_zeros(scene, params):
    """One flat buffer, one view per texture slot: (H, W, 3), or (H, W) for a roughness map."""
    flat = torch.zeros(sum(tex_numel(t) for t in params.tex_shapes), device=scene.device, dtype=torch.float32)
    views, o = [], 0
    for t in params.tex_shapes:
        views.append(flat[o: o + tex_numel(t)].view(tex_view(t)))
        o += tex_numel(t)
    return flat, views


def _texel_tangent(scene, params):
    """Per slot: the bitmap's tangent (``ParamGrads.texture``) times its scale."""
    return [(_f32(params.texture(k), scene.device) * scene.texture_scale(k)).contiguous() for k in range(len(params.tex_shapes))]


def _texel_deposit(scene, params, views):
    for k, v in enumerate(views):
        params.texture(k).add_(v, alpha=scene.texture_scale(k))       # (an envmap's: w.r.t. the bitmap before its scale)


def _alpha_check(scene, params, what):
    n = scene._alpha_slot_count()                                     # (refuses more than EPSM_MAX_ALPHA_GRADS)
    if params.B < n:
        raise ValueError("roughness slots are attached: the gradient buffer must come from Scene.param_grads() after attach_alpha")


def _alpha_zeros(scene, params):
    z = torch.zeros(len(scene.alpha_slots), device=scene.device, dtype=torch.float32)
    return z, z


def _alpha_tangent(scene, params):
    return _f32(params.alpha[:len(scene.alpha_slots)], scene.device).contiguous()


def _alpha_deposit(scene, params, d_alpha):
    params.alpha[:len(scene.alpha_slots)] += d_alpha.to(params.alpha.device)


def _conductor_check(scene, params, what):
    if params.conductor is None or params.M < len(scene.material_slots):
        raise ValueError("conductor materials are attached: the gradient buffer must come from Scene.param_grads() after "
                         "attach_conductor")


def _conductor_zeros(scene, params):
    z = torch.zeros((len(scene.material_slots), 3, 3), device=scene.device, dtype=torch.float32)
    return z, z


def _conductor_tangent(scene, params):
    return _f32(params.conductor[:len(scene.material_slots)], scene.device).contiguous()


def _conductor_deposit(scene, params, d_mat):
    params.conductor[:len(scene.material_slots)] += d_mat.to(params.conductor.device)


def _pose_check(scene, params, what):
    if params.env_pose is None:
        raise ValueError("the envmap's pose is attached: the gradient buffer must come from Scene.param_grads() after "
                         "attach_envmap_pose")


def _pose_zeros(scene, params):
    z = torch.zeros(4, device=scene.device, dtype=torch.float32)
    return z, z


def _pose_tangent(scene, params):
    t = _f32(params.env_pose, scene.device).clone()                   # [omega, ln(scale)]: d ln(scale) = d scale / scale
    t[3] /= scene.envmap_pose()[1]
    return t


def _pose_deposit(scene, params, d_pose):
    d_pose[3] /= scene.envmap_pose()[1]                               # (the ABI's number is d / d ln(scale))
    params.env_pose += d_pose.to(params.env_pose.device)


@dataclass(frozen=True)
class Section:
    name: str
    check: Callable
    zeros: Callable
    tangent: Callable
    deposit: Callable


TEXELS = Section("texels", _texel_check, _texel_zeros, _texel_tangent, _texel_deposit)
ALPHA_SECTION = Section("alpha", _alpha_check, _alpha_zeros, _alpha_tangent, _alpha_deposit)
CONDUCTOR = Section("conductor", _conductor_check, _conductor_zeros, _conductor_tangent, _conductor_deposit)
ENV_POSE = Section("env_pose", _pose_check, _pose_zeros, _pose_tangent, _pose_deposit)


# -- replays: attached(scene) -> is the kind attached; args(scene, buf) asserts that ``buf`` (a section's buffer or tangent) is
#    what the entry points read or write and returns their own arguments, of the ctypes ``own`` ------------------------------
def _is_f32(scene, t, shape=None):
    assert t.is_contiguous() and t.dtype == torch.float32 and t.device.type == scene.device.type
    assert shape is None or tuple(t.shape) == shape


def _texture_args(scene, bufs):
    return scene._texture_pointers(bufs)


def _alpha_texture_args(scene, bufs):
    return scene._texture_pointers(bufs, alpha=True)[:1]


def _alpha_args(scene, buf):
    B = scene._alpha_slot_count()
    _is_f32(scene, buf)
    assert buf.numel() == B
    return buf, int(B)


def _material_args(scene, buf):
    M = len(scene.material_slots)
    _is_f32(scene, buf, (M, 3, 3))
    return buf, int(M)


def _envpose_args(scene, buf):
    _is_f32(scene, buf, (4,))
    return (buf,)


@dataclass(frozen=True)
class Replay:
    name: str                       # Scene.trace_<name>_{backward,forward}
    stem: str                       # epsm_trace_paths_<stem>_{backward,forward}
    own: tuple                      # the ctypes of the kind's own arguments (``args``), the same in both directions
    workspace: Optional[str]        # the *_workspace_bytes entry of the backward pass, if it takes a workspace
    reduces: bool                   # backward reduces without atomics: such a call repeats bit for bit, given exact film weights
    section: Section
    attached: Callable
    args: Callable

    def entry(self, direction: str) -> str:
        return f"epsm_trace_paths_{self.stem}_{direction}"

    def tail(self, direction: str) -> list:
        """The ctypes behind ``radiance``: backward adj_radiance, own[, workspace, bytes], stream; forward own, d_radiance, stream."""
        if direction == "forward":
            return [*self.own, C.c_void_p, C.c_void_p]
        return [C.c_void_p, *self.own, *((C.c_void_p, C.c_size_t) if self.workspace else ()), C.c_void_p]


_P, _SLOTS = C.c_void_p, (C.c_void_p, C.c_int)
TEXTURE = Replay("texture", "texture", (_P, _P), None, False, TEXELS,
                 lambda scene: len(scene.texture_slots) > len(scene.alpha_map_slots()), _texture_args)
ALPHA_TEXTURE = Replay("alpha_texture", "alpha_texture", (_P,), None, False, TEXELS,
                       lambda scene: bool(scene.alpha_map_slots()), _alpha_texture_args)
ALPHA = Replay("alpha", "bsdf", _SLOTS, "epsm_trace_bsdf_workspace_bytes", True, ALPHA_SECTION,
               lambda scene: bool(scene.alpha_slots), _alpha_args)
MATERIAL = Replay("material", "material", _SLOTS, "epsm_trace_material_workspace_bytes", True, CONDUCTOR,
                  lambda scene: bool(scene.material_slots), _material_args)
ENVPOSE = Replay("envpose", "envpose", (_P,), "epsm_trace_envpose_workspace_bytes", True, ENV_POSE,
                 lambda scene: scene.env_pose_attached, _envpose_args)
REPLAYS = (TEXTURE, ALPHA_TEXTURE, ALPHA, MATERIAL, ENVPOSE)


def attached(scene) -> list:
    """The replays attached on ``scene``, in the order of ``REPLAYS``."""
    return [r for r in REPLAYS if r.attached(scene)]


def sections(active) -> list:
    """The sections of the replays ``active``, each once, in their order."""
    return list(dict.fromkeys(r.section for r in active))
