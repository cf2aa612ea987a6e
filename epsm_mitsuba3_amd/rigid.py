"""Rigid motions of vertex ranges: ``epsm_rigid_reduce`` / ``epsm_rigid_expand`` (include/epsm_trace.h, csrc/epsm_trace_rigid.hip).

A slot is a vertex range [lo, hi) and a pivot c.  ``reduce`` turns the per-vertex gradient rows into the slot's [force, torque]
    F = sum_v g_pos[v],    T = sum_v (x_v - c) x g_pos[v] + n_v x g_nrm[v]
-- the gradient of its twist [translation, rotation about c] -- and ``expand`` is the transpose: the vertex motion
    dx_v += dt + dw x (x_v - c),    dn_v += dw x n_v
under the twists, summed over every slot that contains the vertex.  On the GPU these are the two HIP entry points; the torch
forms below are what they are checked against (tests/test_gpu_rigid.py) and what the host build of the tracer runs with
(``host=True``: Scene._backend).  A CPU tensor without that is refused: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

_workspace = {}        # (device, stream) -> the reduce's chunk rows, grown on demand


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"rigid: {what} must be a contiguous float32 tensor")
    return t


def _same_device(positions: torch.Tensor, **tensors) -> None:
    """A pointer of another device must never reach a kernel: refused here."""
    for name, t in tensors.items():
        if t is not None and t.device != positions.device:
            raise ValueError(f"rigid: {name} lives on {t.device}, positions on {positions.device}")


def _tables(ranges: torch.Tensor, pivots: torch.Tensor):
    if ranges.dtype != torch.int64 or ranges.dim() != 2 or ranges.shape[1] != 2 or not ranges.is_contiguous():
        raise ValueError("rigid: ranges must be a contiguous (n, 2) int64 tensor")
    n = int(ranges.shape[0])
    if tuple(pivots.shape) != (n, 3):
        raise ValueError("rigid: pivots must be (n, 3)")
    return n, _f32(pivots, "pivots")


def reduce(positions, normals, g_pos, g_nrm: Optional[torch.Tensor], ranges, pivots, out, host: bool = False) -> None:
    """``out (n,6) += [F, T]``; float64 sums in a fixed order, two calls add the same bits."""
    n, pivots = _tables(ranges, pivots)
    V = int(positions.shape[0])
    if tuple(out.shape) != (n, 6) or tuple(g_pos.shape) != (V, 3) or (g_nrm is not None and tuple(g_nrm.shape) != (V, 3)):
        raise ValueError("rigid.reduce: out must be (n, 6), the gradient rows (V, 3)")
    _same_device(positions, normals=normals if g_nrm is not None else None, g_pos=g_pos, g_nrm=g_nrm, ranges=ranges, pivots=pivots, out=out)
    if not positions.is_cuda:
        if not host:
            raise _lib.EpsmError("epsm_rigid_reduce runs on the GPU only (no CPU fallback)")
        out += reduce_torch(positions, normals, g_pos, g_nrm, ranges, pivots).to(out.dtype)
        return
    lib, dev = _lib.lib(), positions.device
    stream = _lib.stream(dev)
    need = int(lib.epsm_rigid_workspace_bytes(V, n))
    ws = _workspace.get((dev, stream))
    if ws is None or ws.numel() < need:
        ws = _workspace[(dev, stream)] = torch.empty(max(need, 48), device=dev, dtype=torch.uint8)
    ptr = lambda t: None if t is None else C.c_void_p(_f32(t, "a row buffer").data_ptr())
    _lib.check(lib.epsm_rigid_reduce(ptr(positions), ptr(normals), ptr(g_pos), ptr(g_nrm), V, C.c_void_p(ranges.data_ptr()), ptr(pivots), n,
                                     ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(stream)), "epsm_rigid_reduce")


def expand(positions, normals, ranges, pivots, twists, d_pos, d_nrm: Optional[torch.Tensor], host: bool = False) -> None:
    """``d_pos`` / ``d_nrm`` (V,3) += the motion under ``twists (n,6)`` = [dt, dw]."""
    n, pivots = _tables(ranges, pivots)
    V = int(positions.shape[0])
    if tuple(twists.shape) != (n, 6) or tuple(d_pos.shape) != (V, 3) or (d_nrm is not None and tuple(d_nrm.shape) != (V, 3)):
        raise ValueError("rigid.expand: twists must be (n, 6), the tangent rows (V, 3)")
    _same_device(positions, normals=normals if d_nrm is not None else None, ranges=ranges, pivots=pivots, twists=twists, d_pos=d_pos, d_nrm=d_nrm)
    if not positions.is_cuda:
        if not host:
            raise _lib.EpsmError("epsm_rigid_expand runs on the GPU only (no CPU fallback)")
        dp, dn = expand_torch(positions, normals, ranges, pivots, twists)
        d_pos += dp.to(d_pos.dtype)
        if d_nrm is not None:
            d_nrm += dn.to(d_nrm.dtype)
        return
    lib = _lib.lib()
    ptr = lambda t: None if t is None else C.c_void_p(_f32(t, "a row buffer").data_ptr())
    _lib.check(lib.epsm_rigid_expand(ptr(positions), ptr(normals), V, C.c_void_p(ranges.data_ptr()), ptr(pivots), ptr(twists), n, ptr(d_pos),
                                     ptr(d_nrm), C.c_void_p(_lib.stream(positions.device))), "epsm_rigid_expand")


def _clip(ranges: torch.Tensor, V: int):
    for lo, hi in ranges.tolist():
        lo = min(max(lo, 0), V)
        yield lo, min(max(hi, lo), V)


def reduce_torch(positions, normals, g_pos, g_nrm, ranges, pivots) -> torch.Tensor:
    """``reduce`` as dense float64 torch operations: the (n, 6) float64 rows [F, T]."""
    out = torch.zeros((ranges.shape[0], 6), dtype=torch.float64, device=positions.device)
    for s, (lo, hi) in enumerate(_clip(ranges, int(positions.shape[0]))):
        g = g_pos[lo:hi].double()
        out[s, :3] = g.sum(dim=0)
        out[s, 3:] = torch.linalg.cross(positions[lo:hi].double() - pivots[s].double(), g, dim=1).sum(dim=0)
        if g_nrm is not None:
            out[s, 3:] += torch.linalg.cross(normals[lo:hi].double(), g_nrm[lo:hi].double(), dim=1).sum(dim=0)
    return out


def expand_torch(positions, normals, ranges, pivots, twists):
    """``expand`` as dense float64 torch operations: the (V, 3) float64 tangents of positions and normals."""
    d_pos = torch.zeros(positions.shape, dtype=torch.float64, device=positions.device)
    d_nrm = torch.zeros_like(d_pos)
    for s, (lo, hi) in enumerate(_clip(ranges, int(positions.shape[0]))):
        t, w = twists[s, :3].double(), twists[s, 3:].double()
        d_pos[lo:hi] += t + torch.linalg.cross(w.expand(hi - lo, 3), positions[lo:hi].double() - pivots[s].double(), dim=1)
        d_nrm[lo:hi] += torch.linalg.cross(w.expand(hi - lo, 3), normals[lo:hi].double(), dim=1)
    return d_pos, d_nrm
