"""Scene-parameter gradient buffers (what ``dr.grad(params[...])`` holds in the
reference after ``render_backward``, epsm.py:84-306).

All buffers are views into ONE flat fp32 allocation so that a multi-GPU backward
pass needs a single RCCL all-reduce, with no packing copies.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch


def tex_shape(t) -> tuple:
    """An entry of ``tex_shapes`` as ints: (H, W) -- three channels -- or (H, W, 1) -- a roughness map."""
    t = tuple(int(x) for x in t)
    if len(t) not in (2, 3) or (len(t) == 3 and t[2] != 1):
        raise ValueError(f"tex_shapes: an entry is (H, W) -- three channels -- or (H, W, 1) -- a roughness map --, not {t}")
    return t


def tex_numel(t: tuple) -> int:
    """Floats of the section of a ``tex_shapes`` entry."""
    return t[0] * t[1] * (3 if len(t) == 2 else 1)


def tex_view(t: tuple) -> tuple:
    """The shape of the view of a ``tex_shapes`` entry's section: (H, W, 3), or (H, W) for a roughness map."""
    return (t[0], t[1], 3) if len(t) == 2 else (t[0], t[1])


class ParamGrads:
    """``pos (V,3)``: d/d vertex_positions; ``nrm (V,3)``: d/d vertex_normals;
    ``alpha (B)``: d/d per-BSDF roughness; ``cam_origin (3)``: d/d ray origin
    (epsm.py:260-261); ``color (C,3)``: d/d the attached colour parameters (PRBIntegrator); ``texture(slot) (H,W,3)``: d/d the
    texels of an attached bitmap (``Scene.attach_texture``), one section per entry of ``tex_shapes`` at the END of ``flat`` -- every
    other offset, and the buffer of a scene without textures, are what they are without them.  An entry of ``tex_shapes`` is
    ``(H, W)``: three channels, a section of 3 H W floats -- or ``(H, W, 1)``: a roughness map (``'<bsdf>.alpha.data'``), a section of
    H W floats whose ``texture(slot)`` is (H, W); a buffer built with pairs alone has the size and the offsets it always had.  ``rigid (R,6)``: d/d the twist
    [translation, rotation about the slot's pivot] of the rigid slots (``Scene.attach_rigid``) as [force, torque];
    ``cam_rotation (3)``: d/d omega of ``to_world <- Rot(omega) to_world`` about the sensor's own position, world axes, at omega = 0
    (``Scene.attach_sensor(rotation=True)``).  These two sections exist only when asked for (``n_rigid``, ``cam_rotation``; None
    otherwise) and follow the textures: a buffer constructed without them has the size and the offsets it always had.
    ``conductor (M,3,3)``: d/d [eta, k, specular_reflectance] x rgb of the material slots (``Scene.attach_conductor``), likewise
    only when asked for (``n_conductors``), after ``cam_rotation``.  ``env_rotation (3)``, ``env_scale (1)``: d/d omega of the
    envmap's ``to_world <- Rot(omega) to_world`` (world axes, at omega = 0) and d/d its ``scale`` (``Scene.attach_envmap_pose``),
    four floats at the very END, after ``conductor``, only when asked for (``env_pose``; None otherwise).  Vertex
    indices are global: meshes are concatenated and a mesh's rows are ``pos[offset : offset + n_vertices]`` (see ``mesh_slices``)."""

    def __init__(self, n_vertices: int, n_bsdfs: int = 0, device="cuda", mesh_slices: Optional[dict] = None, n_colors: int = 0,
                 tex_shapes: Optional[Sequence[Tuple[int, int]]] = None, n_rigid: int = 0, cam_rotation: bool = False,
                 n_conductors: int = 0, env_pose: bool = False):
        self.V, self.B, self.C = int(n_vertices), int(n_bsdfs), int(n_colors)
        self.tex_shapes = [tex_shape(t) for t in (tex_shapes or [])]
        n0 = 6 * self.V + self.B + 3 + 3 * self.C
        self.R, self.has_cam_rotation = int(n_rigid), bool(cam_rotation)
        n1 = n0 + sum(tex_numel(t) for t in self.tex_shapes)
        n = n1 + 6 * self.R + (3 if self.has_cam_rotation else 0)
        self.M = int(n_conductors)
        self.has_env_pose = bool(env_pose)
        n2 = n + 9 * self.M
        self.flat = torch.zeros(n2 + (4 if self.has_env_pose else 0), device=device, dtype=torch.float32)
        self.pos = self.flat[: 3 * self.V].view(self.V, 3)
        self.nrm = self.flat[3 * self.V: 6 * self.V].view(self.V, 3)
        self.alpha = self.flat[6 * self.V: 6 * self.V + self.B]
        self.cam_origin = self.flat[6 * self.V + self.B: 6 * self.V + self.B + 3]
        # colour parameters of the hybrid scheme's second phase (diffuse reflectances, emitter radiances): (C,3)
        self.color = self.flat[6 * self.V + self.B + 3: n0].view(self.C, 3)
        self._tex, o = [], n0
        for t in self.tex_shapes:
            self._tex.append(self.flat[o: o + tex_numel(t)].view(tex_view(t)))
            o += tex_numel(t)
        self.rigid = self.flat[n1: n1 + 6 * self.R].view(self.R, 6) if self.R else None
        self.cam_rotation = self.flat[n1 + 6 * self.R: n] if self.has_cam_rotation else None
        self.conductor = self.flat[n: n2].view(self.M, 3, 3) if self.M else None
        self.env_pose = self.flat[n2: n2 + 4] if self.has_env_pose else None       # [env_rotation, env_scale]
        self.env_rotation = self.flat[n2: n2 + 3] if self.has_env_pose else None
        self.env_scale = self.flat[n2 + 3: n2 + 4] if self.has_env_pose else None
        self.mesh_slices = dict(mesh_slices or {})
        self._scratch: Optional[ParamGrads] = None             # scratch(): allocated on first use

    def zero_(self):
        self.flat.zero_()
        return self

    def scratch(self) -> "ParamGrads":
        """A zeroed buffer of the same layout (allocated once, cleared on every call): what ONE backward pass
        contributes before it is summed over the ranks and added to the accumulated gradients."""
        s = self._scratch
        if s is None:
            s = self._scratch = ParamGrads(self.V, self.B, device=self.flat.device, mesh_slices=self.mesh_slices, n_colors=self.C,
                                           tex_shapes=self.tex_shapes, n_rigid=self.R, cam_rotation=self.has_cam_rotation,
                                           n_conductors=self.M, env_pose=self.has_env_pose)
        return s.zero_()

    def texture(self, slot: int) -> torch.Tensor:
        """(H, W, 3) view of texture slot ``slot`` (``Scene.attach_texture``): d/d the bitmap the user gave; (H, W) for a
        roughness map."""
        return self._tex[slot]

    def mesh_pos(self, name: str) -> torch.Tensor:
        lo, hi = self.mesh_slices[name]
        return self.pos[lo:hi]

    def mesh_nrm(self, name: str) -> torch.Tensor:
        lo, hi = self.mesh_slices[name]
        return self.nrm[lo:hi]
