"""The scene tables built on the device (include/epsm_trace.h: epsm_scene_topology, epsm_vertex_normals, epsm_emitter_tables,
epsm_environment_tables).

``Scene(..., scene_tables="device")`` takes its vertex normals, emitter CDFs, mesh areas and envmap tables from here instead of
numpy, and moves an emitting mesh without a host round trip.  The host tables stay the default.  Every call is asynchronous on
the current stream of the tensors' device; the scratch comes from torch's allocator.

``vertex_normals_backward`` / ``vertex_normals_forward`` (epsm_vertex_normals_backward / _forward) are the derivative of the normals
with respect to the positions, in both directions, for ``Scene.attach(mesh, recomputed_normals=True)``; ``vertex_normals_vjp_torch`` /
``vertex_normals_jvp_torch`` are their float64 twin, what the kernels are checked against and what the host build of the tracer runs."""
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


_workspace = {}        # (device, stream) -> the a_v rows of vertex_normals_backward, grown on demand


def _rows(positions: torch.Tensor, host: bool, what: str, **tensors) -> int:
    """Shape, type and device of the (V,3) float32 row buffers of the normals' derivative; a pointer of another device must
    never reach a kernel.  A CPU tensor passes only with ``host``: there is no CPU fallback."""
    V = int(positions.shape[0])
    for name, t in dict(positions=positions, **tensors).items():
        if t.dtype != torch.float32 or tuple(t.shape) != (V, 3) or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous ({V},3) float32 tensor")
        if t.device != positions.device:
            raise ValueError(f"{what}: {name} lives on {t.device}, positions on {positions.device}")
    if not positions.is_cuda and not host:
        raise _lib.EpsmError(f"epsm_{what} runs on the GPU only (no CPU fallback)")
    return V


def _flagged_runs(meshes, vertex_begin, first: int, count: int):
    """(v0, v1, [(tri_begin, tri_count), ...]) of every run of consecutive meshes flagged EPSM_MESH_VERTEX_NORMALS."""
    runs, m = [], first
    while m < first + count:
        if not meshes[m].flags & 1:
            m += 1
            continue
        v0, tris = int(vertex_begin[m]), []
        while m < first + count and meshes[m].flags & 1:
            tris.append((int(meshes[m].tri_begin), int(meshes[m].tri_count)))
            m += 1
        if int(vertex_begin[m]) > v0:
            runs.append((v0, int(vertex_begin[m]), tris))
    return runs


def _run_faces(tri: torch.Tensor, v0: int, v1: int, tris) -> torch.Tensor:
    f = torch.cat([tri[t0:t0 + n] for t0, n in tris]).long() - v0 if tris else torch.zeros((0, 3), dtype=torch.int64)
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v1 - v0):
        raise ValueError("the float64 twin takes meshes whose triangles name their own vertices")
    return f


def vertex_normals_backward(positions: torch.Tensor, tri: torch.Tensor, meshes, vertex_begin: Sequence[int], g_nrm: torch.Tensor,
                            g_pos: torch.Tensor, topology: SceneTopology = None, first: int = 0, count: int = None,
                            host: bool = False) -> None:
    """``g_pos[w] += sum_v (d n_v / d p_w)^T g_nrm[v]`` (epsm_vertex_normals_backward), in place, for the vertex rows of meshes
    ``first .. first + count`` of the host table ``meshes`` that are flagged EPSM_MESH_VERTEX_NORMALS: the adjoint of
    :func:`vertex_normals`; every other row is left as it is.  No atomics: two calls add the same bits.  ``host=True`` (the
    host build of the tracer, ``Scene._backend``) runs the float64 torch twin :func:`vertex_normals_vjp_torch`."""
    V = _rows(positions, host, "vertex_normals_backward", g_nrm=g_nrm, g_pos=g_pos)
    count = len(meshes) - first if count is None else count
    if not positions.is_cuda:
        for v0, v1, tris in _flagged_runs(meshes, vertex_begin, first, count):
            g_pos[v0:v1] += vertex_normals_vjp_torch(positions[v0:v1].double(), _run_faces(tri, v0, v1, tris), g_nrm[v0:v1].double()).float()
        return
    if topology is None or topology.tri.device != positions.device:
        raise ValueError("vertex_normals_backward: the SceneTopology of the triangles, on the positions' device")
    L, dev = _lib.lib(), positions.device
    stream = _lib.stream(dev)
    need = int(L.epsm_vertex_normals_backward_bytes(V))
    ws = _workspace.get((dev, stream))
    if ws is None or ws.numel() < need:
        ws = _workspace[(dev, stream)] = _scratch(need, dev)
    vb = (C.c_int64 * (count + 1))(*[int(x) for x in vertex_begin[first:first + count + 1]])
    _lib.check(L.epsm_vertex_normals_backward(positions.data_ptr(), V, topology.tri.data_ptr(), topology.T, topology.buf.data_ptr(),
                                              _meshes_at(meshes, first), vb, count, g_nrm.data_ptr(), g_pos.data_ptr(), ws.data_ptr(),
                                              ws.numel(), stream), "epsm_vertex_normals_backward")


def vertex_normals_forward(positions: torch.Tensor, tri: torch.Tensor, meshes, vertex_begin: Sequence[int], d_pos: torch.Tensor,
                           d_nrm: torch.Tensor, topology: SceneTopology = None, first: int = 0, count: int = None,
                           host: bool = False) -> None:
    """``d_nrm[v] += sum_w (d n_v / d p_w) d_pos[w]`` (epsm_vertex_normals_forward), in place: the transpose of
    :func:`vertex_normals_backward` over the same rows; ``host=True`` runs :func:`vertex_normals_jvp_torch`."""
    V = _rows(positions, host, "vertex_normals_forward", d_pos=d_pos, d_nrm=d_nrm)
    count = len(meshes) - first if count is None else count
    if not positions.is_cuda:
        for v0, v1, tris in _flagged_runs(meshes, vertex_begin, first, count):
            d_nrm[v0:v1] += vertex_normals_jvp_torch(positions[v0:v1].double(), _run_faces(tri, v0, v1, tris), d_pos[v0:v1].double()).float()
        return
    if topology is None or topology.tri.device != positions.device:
        raise ValueError("vertex_normals_forward: the SceneTopology of the triangles, on the positions' device")
    vb = (C.c_int64 * (count + 1))(*[int(x) for x in vertex_begin[first:first + count + 1]])
    _lib.check(_lib.lib().epsm_vertex_normals_forward(positions.data_ptr(), V, topology.tri.data_ptr(), topology.T,
                                                      topology.buf.data_ptr(), _meshes_at(meshes, first), vb, count, d_pos.data_ptr(),
                                                      d_nrm.data_ptr(), _lib.stream(positions.device)), "epsm_vertex_normals_forward")


# -- the float64 twin: the vjp / jvp of scene.vertex_normals_torch written out, with the primal's cuts ---------------------------
_FLOOR = 1e-30


def _normals_pieces(v: torch.Tensor, f: torch.Tensor):
    """What both directions share, as the kernels form it: edges, unit face normals and their lengths, per corner the angle and
    d angle / d (its two edges), the vertex sums' unit vectors and lengths.  A derivative is 0 where the primal is cut to a
    constant: a length on its floor (0 or below the 1e-30 of its division), a cosine on or outside [-1, 1]."""
    if v.dtype != torch.float64 or f.dtype != torch.int64:
        raise ValueError("the twin of the normals' derivative takes float64 positions and int64 faces")
    # every product rounded on its own, as the numpy rule and the kernels do: a fused a x a leaves a residue instead of 0, and the
    # normalisation turns that into a unit face normal (csrc/epsm_trace_scene.hip, `mul`)
    cross = lambda a, b: torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    p = v[f]                                                                                # (T,3,3)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    x = cross(e1, e2)
    ln = x.norm(dim=1, keepdim=True)
    fn = torch.where(ln > 0, x / ln.clamp_min(_FLOOR), torch.zeros_like(x))
    face_ok, ln = ln > _FLOOR, ln.clamp_min(_FLOOR)
    ang, g0, g1 = [], [], []
    N = torch.zeros_like(v)
    for i in range(3):
        d0, d1 = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        q0, q1 = (d0 * d0).sum(1, keepdim=True), (d1 * d1).sum(1, keepdim=True)
        den = q0.sqrt() * q1.sqrt()
        cos = (d0 * d1).sum(1, keepdim=True) / den.clamp_min(_FLOOR)
        ok = (den > _FLOOR) & (cos > -1) & (cos < 1)
        one = torch.ones_like(den)
        den, q0, q1, c = torch.where(ok, den, one), torch.where(ok, q0, one), torch.where(ok, q1, one), torch.where(ok, cos, 0 * one)
        s = torch.where(ok, -1.0 / ((1.0 - c) * (1.0 + c)).sqrt(), 0 * one)                # d acos / d cos
        ang.append(torch.acos(cos.clamp(-1, 1)))
        g0.append(s * (d1 / den - c * d0 / q0))
        g1.append(s * (d0 / den - c * d1 / q1))
        N.index_add_(0, f[:, i], fn * ang[-1])
    lv = N.norm(dim=1, keepdim=True)
    vert_ok, lv = lv > _FLOOR, lv.clamp_min(_FLOOR)
    n = torch.where(vert_ok, N / lv, torch.zeros_like(N))
    return cross, e1, e2, fn, ln, face_ok, ang, g0, g1, n, lv, vert_ok


def vertex_normals_vjp_torch(v: torch.Tensor, f: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """``sum_v (d n_v / d p_w)^T g[v]`` of ``scene.vertex_normals`` in float64: (V,3)."""
    cross, e1, e2, fn, ln, face_ok, ang, g0, g1, n, lv, vert_ok = _normals_pieces(v, f)
    a = torch.where(vert_ok, (g - n * (n * g).sum(1, keepdim=True)) / lv, torch.zeros_like(g))
    av = a[f]                                                                               # (T,3,3)
    G = torch.zeros_like(av)
    b = torch.zeros_like(fn)
    for i in range(3):
        s = (av[:, i] * fn).sum(1, keepdim=True)
        b = b + ang[i] * av[:, i]
        G[:, i] -= s * (g0[i] + g1[i])
        G[:, (i + 1) % 3] += s * g0[i]
        G[:, (i + 2) % 3] += s * g1[i]
    gx = torch.where(face_ok, (b - fn * (fn * b).sum(1, keepdim=True)) / ln, torch.zeros_like(b))
    ge1, ge2 = cross(e2, gx), cross(gx, e1)
    G[:, 0] -= ge1 + ge2
    G[:, 1] += ge1
    G[:, 2] += ge2
    return torch.zeros_like(v).index_add_(0, f.reshape(-1), G.reshape(-1, 3))


def vertex_normals_jvp_torch(v: torch.Tensor, f: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """``sum_w (d n_v / d p_w) t[w]`` of ``scene.vertex_normals`` in float64: (V,3)."""
    cross, e1, e2, fn, ln, face_ok, ang, g0, g1, n, lv, vert_ok = _normals_pieces(v, f)
    tp = t[f]
    dx = cross(tp[:, 1] - tp[:, 0], e2) + cross(e1, tp[:, 2] - tp[:, 0])
    df = torch.where(face_ok, (dx - fn * (fn * dx).sum(1, keepdim=True)) / ln, torch.zeros_like(dx))
    dN = torch.zeros_like(v)
    for i in range(3):
        dang = (g0[i] * (tp[:, (i + 1) % 3] - tp[:, i])).sum(1, keepdim=True) + (g1[i] * (tp[:, (i + 2) % 3] - tp[:, i])).sum(1, keepdim=True)
        dN.index_add_(0, f[:, i], dang * fn + ang[i] * df)
    return torch.where(vert_ok, (dN - n * (n * dN).sum(1, keepdim=True)) / lv, torch.zeros_like(dN))


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
