"""The scene tables built on the device (include/epsm_trace.h: epsm_scene_topology, epsm_vertex_normals, epsm_emitter_tables,
epsm_environment_tables).

``Scene(..., scene_tables="device")`` takes its vertex normals, emitter CDFs, mesh areas and envmap tables from here instead of
numpy, and moves an emitting mesh without a host round trip.  The host tables stay the default.  Every call is asynchronous on
the current stream of the tensors' device; the scratch comes from torch's allocator."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import _lib

MESH_BYTES = 32                 # sizeof(EpsmMesh)


def _check(t: torch.Tensor, name: str, dtype, cols: int):
    if t.device.type != "cuda":
        raise ValueError(f"{name}: the device scene tables need tensors on a GPU")
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous (n,{cols}) {dtype} tensor")
    return t


def _scratch(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _meshes_at(meshes, first: int):
    return C.c_void_p(C.addressof(meshes) + first * MESH_BYTES)


class SceneTopology:
    """The vertex -> (triangle, corner) adjacency of ``tri`` ((T,3) int32) over ``V`` vertices (epsm_scene_topology): built once
    per triangle set, read by every :func:`vertex_normals` call."""

    def __init__(self, tri: torch.Tensor, V: int):
        tri = _check(tri, "tri", torch.int32, 3)
        L = _lib.lib()
        self.V, self.T, self.tri = int(V), int(tri.shape[0]), tri
        self.buf = _scratch(L.epsm_scene_topology_bytes(self.V, self.T), tri.device)
        ws_bytes = int(L.epsm_scene_topology_workspace_bytes(self.T))
        ws = _scratch(ws_bytes, tri.device)
        _lib.check(L.epsm_scene_topology(tri.data_ptr(), self.V, self.T, self.buf.data_ptr(), self.buf.numel(), ws.data_ptr(),
                                         ws.numel(), _lib.stream(tri.device)), "epsm_scene_topology")


def vertex_normals(positions: torch.Tensor, topology: SceneTopology, meshes, vertex_begin: Sequence[int], normals: torch.Tensor,
                   first: int = 0, count: int = None) -> None:
    """epsm_vertex_normals into ``normals`` ((V,3) float32, in place) for meshes ``first .. first + count`` of the host table
    ``meshes`` (a ctypes array of EpsmMesh) whose flags carry EPSM_MESH_VERTEX_NORMALS; ``vertex_begin``: the first vertex row of
    every mesh of the table and the end of the last (len(meshes) + 1 entries)."""
    positions = _check(positions, "positions", torch.float32, 3)
    normals = _check(normals, "normals", torch.float32, 3)
    count = len(meshes) - first if count is None else count
    vb = (C.c_int64 * (count + 1))(*[int(x) for x in vertex_begin[first:first + count + 1]])
    _lib.check(_lib.lib().epsm_vertex_normals(positions.data_ptr(), positions.shape[0], topology.tri.data_ptr(), topology.T,
                                              topology.buf.data_ptr(), _meshes_at(meshes, first), vb, count, normals.data_ptr(),
                                              _lib.stream(positions.device)), "epsm_vertex_normals")


def emitter_tables(positions: torch.Tensor, tri: torch.Tensor, meshes, mesh_buf: torch.Tensor, emitter_cdf: torch.Tensor,
                   first: int = 0, count: int = None) -> None:
    """epsm_emitter_tables for meshes ``first .. first + count`` of the host table ``meshes`` (ctypes EpsmMesh array) and its
    device copy ``mesh_buf`` (uint8): their CDFs into ``emitter_cdf`` (float32) and their areas into ``mesh_buf``, in place.
    The host copy's ``area`` fields are not touched."""
    positions = _check(positions, "positions", torch.float32, 3)
    tri = _check(tri, "tri", torch.int32, 3)
    count = len(meshes) - first if count is None else count
    if mesh_buf.dtype != torch.uint8 or mesh_buf.numel() < (first + count) * MESH_BYTES:
        raise ValueError("mesh_buf: the device mesh table (uint8)")
    if emitter_cdf.dtype != torch.float32 or not emitter_cdf.is_contiguous():
        raise ValueError("emitter_cdf: a contiguous float32 tensor")
    L = _lib.lib()
    T = int(tri.shape[0])
    ws = _scratch(L.epsm_emitter_tables_bytes(T, count), positions.device)
    _lib.check(L.epsm_emitter_tables(positions.data_ptr(), positions.shape[0], tri.data_ptr(), T, _meshes_at(meshes, first),
                                     mesh_buf.data_ptr() + first * MESH_BYTES, count, emitter_cdf.data_ptr(), emitter_cdf.numel(),
                                     ws.data_ptr(), ws.numel(), _lib.stream(positions.device)), "epsm_emitter_tables")


def environment_tables(bitmap: torch.Tensor):
    """epsm_environment_tables of an (H, W, 3) float32 map on the device -> texels (H, W + 1, 3), row_cdf (H - 1),
    col_cdf (H - 1, W), cell_pdf (H - 1, W): the arrays of scene.environment_tables, as float32 device tensors."""
    if bitmap.device.type != "cuda" or bitmap.dtype != torch.float32 or bitmap.dim() != 3 or bitmap.shape[2] != 3:
        raise ValueError("bitmap: an (H, W, 3) float32 tensor on a GPU")
    bitmap = bitmap.contiguous()
    H, W = int(bitmap.shape[0]), int(bitmap.shape[1])
    dev = bitmap.device
    texels = torch.empty((H, W + 1, 3), dtype=torch.float32, device=dev)
    row_cdf = torch.empty(max(H - 1, 0), dtype=torch.float32, device=dev)
    col_cdf = torch.empty((max(H - 1, 0), W), dtype=torch.float32, device=dev)
    cell_pdf = torch.empty((max(H - 1, 0), W), dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = _scratch(L.epsm_environment_tables_bytes(W, H), dev)
    _lib.check(L.epsm_environment_tables(bitmap.data_ptr(), W, H, texels.data_ptr(), row_cdf.data_ptr(), col_cdf.data_ptr(),
                                         cell_pdf.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream(dev)), "epsm_environment_tables")
    return texels, row_cdf, col_cdf, cell_pdf
