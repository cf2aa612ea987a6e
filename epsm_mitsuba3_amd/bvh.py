"""The four-wide BVH built and refitted on the device (include/epsm_trace.h: epsm_bvh_build / epsm_bvh_refit).

``Scene(..., bvh_builder="device")`` uses :class:`NativeBvh` in place of the host builder (scene.build_bvh + DeviceBvh):
same node format, same depth bound, same boxes for the same tree.  The host builder stays the default."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np
import torch

from . import _lib

MAX_WIDE_LEVELS = 16            # scene.kMaxWideDepth
ABSENT = 0x7fffffff


def _checked_inputs(positions: torch.Tensor, tri: torch.Tensor):
    if positions.device.type != "cuda" or tri.device.type != "cuda":
        raise ValueError("the device BVH needs positions and triangles on a GPU")
    if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] != 3 or not positions.is_contiguous():
        raise ValueError("positions: a contiguous (V,3) float32 tensor")
    if tri.dtype != torch.int32 or tri.dim() != 2 or tri.shape[1] != 3 or not tri.is_contiguous():
        raise ValueError("tri: a contiguous (T,3) int32 tensor")
    return positions, tri


def level_table(nodes: np.ndarray) -> List[int]:
    """``level_begin`` of a breadth-first tree of ``EpsmBvhNode`` rows ((n,32) float32, e.g. build_bvh()["nodes"]): wide
    level l is rows [level_begin[l], level_begin[l + 1])."""
    c = np.ascontiguousarray(nodes, dtype=np.float32).view(np.int32)[:, 24:28]
    begin, frontier = [0], np.zeros(1, dtype=np.int64)
    while frontier.size:
        kids = c[frontier].reshape(-1)
        kids = kids[(kids >= 0) & (kids != ABSENT)].astype(np.int64)
        if kids.size and (kids.min() != frontier.max() + 1 or kids.max() != frontier.max() + kids.size):
            raise ValueError("the tree is not in breadth-first order")
        begin.append(int(frontier.max()) + 1)
        frontier = kids
    return begin


def refit(nodes: torch.Tensor, prim_index: torch.Tensor, tri_verts: torch.Tensor, level_begin: Sequence[int],
          positions: torch.Tensor, tri: torch.Tensor) -> None:
    """epsm_bvh_refit of any breadth-first tree in place: ``nodes`` (n,32) float32, ``prim_index`` (T) int32, ``tri_verts`` (T,9)
    float32, all on the device of ``positions``."""
    positions, tri = _checked_inputs(positions, tri)
    n_levels = len(level_begin) - 1
    lb = (C.c_int32 * (n_levels + 1))(*level_begin)
    rc = _lib.lib().epsm_bvh_refit(positions.data_ptr(), positions.shape[0], tri.data_ptr(), prim_index.data_ptr(), tri.shape[0],
                                   nodes.data_ptr(), nodes.shape[0], lb, n_levels, tri_verts.data_ptr(), _lib.stream(positions.device))
    _lib.check(rc, "epsm_bvh_refit")


class NativeBvh:
    """The tree of epsm_bvh_build and its refit, with the attributes the scene struct reads from DeviceBvh: ``nodes`` (n,32)
    float32, ``prim_index`` (T) int32, ``tri_verts`` (T,9) float32; ``level_begin`` the wide levels' first rows (n_levels + 1
    entries).  ``refit`` writes into these tensors: the scene struct keeps their pointers."""

    def __init__(self, positions: torch.Tensor, tri: torch.Tensor):
        positions, tri = _checked_inputs(positions, tri)
        L = _lib.lib()
        dev = positions.device
        V, T = positions.shape[0], tri.shape[0]
        if T < 1:
            raise ValueError("the device BVH needs at least one triangle")
        cap = int(L.epsm_bvh_max_nodes(T))
        nodes = torch.empty((cap, 32), dtype=torch.float32, device=dev)
        self.prim_index = torch.empty(T, dtype=torch.int32, device=dev)
        self.tri_verts = torch.empty((T, 9), dtype=torch.float32, device=dev)
        ws_bytes = int(L.epsm_bvh_workspace_bytes(T))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        n_nodes, n_levels = C.c_int32(0), C.c_int32(0)
        lb = (C.c_int32 * (MAX_WIDE_LEVELS + 1))()
        rc = L.epsm_bvh_build(positions.data_ptr(), V, tri.data_ptr(), T, nodes.data_ptr(), self.prim_index.data_ptr(),
                              self.tri_verts.data_ptr(), C.byref(n_nodes), lb, C.byref(n_levels), ws.data_ptr(), ws_bytes,
                              _lib.stream(dev))
        _lib.check(rc, "epsm_bvh_build")
        del ws
        self.nodes = nodes[:n_nodes.value].clone()
        self.level_begin = [int(lb[i]) for i in range(n_levels.value + 1)]

    @property
    def n_levels(self) -> int:
        return len(self.level_begin) - 1

    def refit(self, positions: torch.Tensor, tri: torch.Tensor):
        """positions (V,3) f32, tri (T,3) int32 -> tri_verts in leaf order and fresh boxes, in place (asynchronous)."""
        refit(self.nodes, self.prim_index, self.tri_verts, self.level_begin, positions, tri)


def sah_cost(nodes) -> float:
    """SAH cost of a four-wide tree from its boxes: sum over the wide nodes of SA(node) / SA(root) plus sum over the leaf slots of
    count SA(leaf) / SA(root) (SA of a node: the box around its four slots)."""
    a = (nodes.detach().cpu().numpy() if torch.is_tensor(nodes) else np.asarray(nodes)).astype(np.float32)
    c = a.view(np.int32)[:, 24:28]
    cnt = a.view(np.int32)[:, 28:32]
    lo = a[:, 0:12].reshape(-1, 3, 4).astype(np.float64)
    hi = a[:, 12:24].reshape(-1, 3, 4).astype(np.float64)

    def area(l, h):
        d = np.maximum(h - l, 0.0)
        return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])

    present = c != ABSENT
    nlo = np.where(present[:, None, :], lo, np.inf).min(axis=2)
    nhi = np.where(present[:, None, :], hi, -np.inf).max(axis=2)
    node_sa = area(nlo, nhi)
    leaf = present & (c < 0)
    slot_sa = area(np.moveaxis(lo, 1, 2), np.moveaxis(hi, 1, 2))       # (n,4)
    return float((node_sa.sum() + (cnt * slot_sa)[leaf].sum()) / node_sa[0])
