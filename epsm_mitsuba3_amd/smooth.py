"""Large-steps vertex updates: ``epsm_mesh_laplacian`` / ``epsm_laplacian_apply`` / ``epsm_laplacian_solve``
(include/epsm_trace.h, csrc/epsm_trace_smooth.hip).

Nicolet, Jakob and Jacobson (2021) optimise ``u = (I + lam L) x`` instead of the vertices ``x`` of a mesh, L its combinatorial
Laplacian: the gradient of ``u`` is ``(I + lam L)^-1 g_x``, a smooth displacement field where ``g_x`` -- a Monte Carlo gradient,
confined to silhouettes and caustic footprints -- is sparse and noisy.  :class:`MeshLaplacian` is that matrix on the device, with
the product, the conjugate-gradient solve and the differentiable ``from_differential``; :class:`AdamUniform` is the paper's
optimiser.  On the GPU these are the HIP entry points; the torch forms below (``laplacian_dense``, ``apply_torch``,
``solve_torch``) are what they are checked against and what ``host=True`` runs (the host build of the tracer, ``Scene._backend``).
A CPU tensor without that is refused: there is no CPU fallback.

Multi-rank runs need nothing of their own: the solve runs after the all-reduce of ``ParamGrads`` and is bit-repeatable, so the
ranks stay identical."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib

FORMS = {"auto": 0, "grid": 1, "one_group": 2}           # include/epsm_trace.h EPSM_SMOOTH_*
ONE_GROUP_MAX_V = 13312                                   # EPSM_SMOOTH_ONE_GROUP_MAX_V

_workspace = {}        # (device, stream) -> the solve's vectors and chunk rows, grown on demand


class EpsmSmoothInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("residual", C.c_double)]


# -- the torch forms -----------------------------------------------------------------------------------------------------------
def unique_edges(tri: torch.Tensor, V: int) -> torch.Tensor:
    """The undirected edges {v, w}, v < w, that some triangle of ``tri`` (T,3) has, each once: (E,2) int64, sorted.  A triangle
    naming a vertex twice gives no self-edge; an entry outside 0 .. V - 1 gives no edge."""
    f = tri.long().reshape(-1, 3)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = e[(e[:, 0] != e[:, 1]) & (e >= 0).all(1) & (e < V).all(1)]
    e = torch.stack([e.min(1).values, e.max(1).values], 1)
    return torch.unique(e, dim=0)


def laplacian_dense(tri: torch.Tensor, V: int) -> torch.Tensor:
    """L as a dense (V,V) float64 matrix: -1 per unique edge, the number of distinct neighbours on the diagonal."""
    e = unique_edges(tri, V)
    L = torch.zeros((V, V), dtype=torch.float64, device=tri.device)
    L[e[:, 0], e[:, 1]] = -1.0
    L[e[:, 1], e[:, 0]] = -1.0
    L[torch.arange(V), torch.arange(V)] = -L.sum(1)
    return L


def apply_torch(edges: torch.Tensor, degree: torch.Tensor, lam: float, x: torch.Tensor) -> torch.Tensor:
    """``(I + lam L) x`` from the unique edges and the degrees, in x's dtype."""
    s = torch.zeros_like(x).index_add_(0, edges[:, 0], x[edges[:, 1]]).index_add_(0, edges[:, 1], x[edges[:, 0]])
    return x + lam * (degree.to(x.dtype)[:, None] * x - s)


def solve_torch(edges, degree, lam: float, b: torch.Tensor, x0: Optional[torch.Tensor], rel_tol: float, max_iters: int):
    """Conjugate gradients on ``(I + lam L) x = b`` in float64, column by column state as the kernels keep it:
    (x in b's dtype, [(iterations, converged, |r| / |b|)] per column)."""
    b64 = b.double()
    x = torch.zeros_like(b64) if x0 is None else x0.double().clone()
    A = lambda p: apply_torch(edges, degree, lam, p)
    r = b64 - A(x)
    bb, rr = (b64 * b64).sum(0), (r * r).sum(0)
    zero = bb == 0
    rel = torch.where(zero, torch.zeros_like(rr), (rr / bb.clamp_min(1e-300)).sqrt())
    active = ~zero & ~(rel <= rel_tol)
    iters = torch.zeros(b.shape[1], dtype=torch.int64)
    p = r.clone()
    for k in range(1, max_iters + 1):
        if not bool(active.any()):
            break
        q = A(p)
        pq = (p * q).sum(0)
        alpha = torch.where(active & (pq != 0), rr / torch.where(pq != 0, pq, torch.ones_like(pq)), torch.zeros_like(pq))
        x, r = x + alpha * p, r - alpha * q
        rr_new = torch.where(active, (r * r).sum(0), rr)
        rel = torch.where(active, (rr_new / bb.clamp_min(1e-300)).sqrt(), rel)
        iters = torch.where(active.cpu(), torch.full_like(iters, k), iters)
        active = active & ~(rel <= rel_tol)
        beta = torch.where(active, rr_new / rr.clamp_min(1e-300), torch.zeros_like(rr))
        rr = rr_new
        p = r + beta * p
    x[:, zero] = 0.0
    info = [(int(iters[c]), bool(zero[c]) or float(rel[c]) <= rel_tol, float(rel[c])) for c in range(b.shape[1])]
    return x.to(b.dtype), info


# -- the matrix ----------------------------------------------------------------------------------------------------------------
class _FromDifferential(torch.autograd.Function):
    """x = (I + lam L)^-1 u; the matrix is symmetric, so the backward pass is the same solve of the incoming gradient."""

    @staticmethod
    def forward(ctx, u, lap, kwargs):
        ctx.lap, ctx.kwargs = lap, kwargs
        return lap.solve(u.detach(), **kwargs)

    @staticmethod
    def backward(ctx, g):
        return ctx.lap.solve(g.contiguous(), **ctx.kwargs), None, None


class MeshLaplacian:
    """``I + lam L`` of the triangles ``tri`` ((T,3) int32, indices into the mesh's own ``V`` vertices) on ``tri``'s device, L the
    unique-edge combinatorial Laplacian: -1 for every undirected edge some triangle has -- once, however many triangles share
    it -- and the number of distinct neighbours on the diagonal.  Rebuild it when the triangles change, not when the vertices
    move.  Reading ``max_degree`` back at the end of the build is the object's one host synchronisation.

    Vertices duplicated along a UV seam are boundary to L: the two copies share no edge, so the smoothing does not cross the
    seam and the copies may drift apart.  Welding them is the caller's business; nothing here welds.

    ``apply(x)`` / ``to_differential(x)``: ``(I + lam L) x`` for (V,3) float32 rows.  ``solve(b)``: conjugate gradients, see there.
    ``from_differential(u)``: the solve as a ``torch.autograd.Function`` whose backward is the same solve."""

    def __init__(self, tri: torch.Tensor, V: int, lam: float, device=None, host: bool = False):
        lam = float(lam)
        if not math.isfinite(lam) or lam < 0:
            raise ValueError("MeshLaplacian: lam must be finite and >= 0")
        if tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype not in (torch.int32, torch.int64):
            raise ValueError("MeshLaplacian: tri must be a (T,3) int32 tensor")
        if device is not None:
            tri = tri.to(device)
        self.V, self.T, self.lam, self.device, self.host = int(V), int(tri.shape[0]), lam, tri.device, bool(host)
        self._info = None
        if not tri.is_cuda:
            if not host:
                raise _lib.EpsmError("epsm_mesh_laplacian runs on the GPU only (no CPU fallback)")
            self.edges = unique_edges(tri, self.V)
            self.degree = torch.zeros(self.V, dtype=torch.int64).index_add_(0, self.edges.reshape(-1),
                                                                            torch.ones(self.edges.numel(), dtype=torch.int64))
            self.max_degree = int(self.degree.max()) if self.V else 0
            return
        from .scene_tables import SceneTopology
        lib = _lib.lib()
        self.tri = tri.to(torch.int32).contiguous()
        topology = SceneTopology(self.tri, self.V)
        self.table = torch.empty(int(lib.epsm_mesh_laplacian_bytes(self.V, self.T)), dtype=torch.uint8, device=self.device)
        _lib.check(lib.epsm_mesh_laplacian(self.tri.data_ptr(), self.V, self.T, topology.buf.data_ptr(), self.table.data_ptr(),
                                           self.table.numel(), _lib.stream(self.device)), "epsm_mesh_laplacian")
        self._info_buf = torch.zeros(6, dtype=torch.float64, device=self.device)      # 3 x EpsmSmoothInfo
        self.max_degree = int(self.table[:4].view(torch.int32).item())                # (synchronises: once, at build time)

    # the textbook bound of CG, ceil(0.5 sqrt(kappa) ln(2 / rel_tol)), with kappa <= 1 + 2 lam max_degree (Gershgorin)
    def default_max_iters(self, rel_tol: float) -> int:
        kappa = 1.0 + 2.0 * self.lam * self.max_degree
        return max(1, math.ceil(0.5 * math.sqrt(kappa) * math.log(2.0 / rel_tol)))

    def _rows(self, what: str, **tensors):
        for name, t in tensors.items():
            if t is None:
                continue
            if tuple(t.shape) != (self.V, 3) or not t.is_contiguous():
                raise ValueError(f"smooth.{what}: {name} must be a contiguous ({self.V},3) tensor")
            if t.device != self.device:
                raise ValueError(f"smooth.{what}: {name} lives on {t.device}, the Laplacian on {self.device}")
            if self.device.type == "cuda" and t.dtype != torch.float32:
                raise ValueError(f"smooth.{what}: {name} must be float32 on the GPU")

    def apply(self, x: torch.Tensor) -> torch.Tensor:
        """``(I + lam L) x``: each row summed in float64 in table order, rounded to float32 once."""
        self._rows("apply", x=x)
        if self.device.type != "cuda":
            return apply_torch(self.edges, self.degree, self.lam, x)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().epsm_laplacian_apply(self.table.data_ptr(), self.V, self.lam, x.data_ptr(), y.data_ptr(),
                                                        _lib.stream(self.device)), "epsm_laplacian_apply")
        return y

    to_differential = apply

    def solve(self, b: torch.Tensor, x0: Optional[torch.Tensor] = None, rel_tol: float = 1e-6, max_iters: Optional[int] = None,
              form: str = "auto") -> torch.Tensor:
        """``(I + lam L)^-1 b`` by conjugate gradients from ``x0`` (default 0), a column stopping at ``|r| <= rel_tol |b|`` or after
        ``max_iters`` (default: :meth:`default_max_iters`).  Asynchronous on the current stream: the host never learns whether
        the solve converged unless it asks :meth:`info`.  ``form``: "auto", "grid" or "one_group" (V <= 13312)."""
        self._rows("solve", b=b, x0=x0)
        if form not in FORMS:
            raise ValueError(f"smooth.solve: form must be one of {sorted(FORMS)}")
        max_iters = self.default_max_iters(rel_tol) if max_iters is None else int(max_iters)
        if self.device.type != "cuda":
            x, self._info = solve_torch(self.edges, self.degree, self.lam, b, x0, rel_tol, max_iters)
            return x
        lib, dev = _lib.lib(), self.device
        stream = _lib.stream(dev)
        need = int(lib.epsm_laplacian_solve_bytes(self.V))
        ws = _workspace.get((dev, stream))
        if ws is None or ws.numel() < need:
            ws = _workspace[(dev, stream)] = torch.empty(need, dtype=torch.uint8, device=dev)
        x = torch.zeros_like(b) if x0 is None else x0.detach().clone()
        _lib.check(lib.epsm_laplacian_solve(self.table.data_ptr(), self.V, self.lam, b.data_ptr(), x.data_ptr(), max_iters, float(rel_tol),
                                            FORMS[form], self._info_buf.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                   "epsm_laplacian_solve")
        return x

    def from_differential(self, u: torch.Tensor, **solve_kwargs) -> torch.Tensor:
        """``x = (I + lam L)^-1 u``, differentiable: ``x.backward(g)`` leaves ``(I + lam L)^-1 g`` in ``u.grad``."""
        return _FromDifferential.apply(u, self, solve_kwargs)

    def info(self):
        """The last solve's [(iterations, converged, |r| / |b|)] per column.  SYNCHRONISES with the device: it copies the info
        words to the host."""
        if self.device.type != "cuda":
            return self._info
        raw = (EpsmSmoothInfo * 3).from_buffer_copy(self._info_buf.cpu().numpy().tobytes())
        return [(int(i.iterations), bool(i.converged), float(i.residual)) for i in raw]

    def neighbours(self):
        """The rows of the table as Python sets, [set of neighbours of v] (reads the table back: for tests and inspection)."""
        if self.device.type != "cuda":
            rows = [set() for _ in range(self.V)]
            for v, w in self.edges.tolist():
                rows[v].add(w); rows[w].add(v)
            return rows
        align = lambda n: (n + 255) // 256 * 256
        words = self.table.cpu().view(torch.int32)
        o_row = 256 // 4
        o_deg = o_row + align(4 * (self.V + 1)) // 4
        o_nbr = o_deg + align(4 * self.V) // 4
        row, deg = words[o_row:o_row + self.V + 1].tolist(), words[o_deg:o_deg + self.V].tolist()
        out = []
        for v in range(self.V):
            slots = words[o_nbr + 2 * row[v]:o_nbr + 2 * row[v + 1]].tolist()
            kept = [w for w in slots if w != -1]
            if len(kept) != deg[v] or slots[:deg[v]] != kept:
                raise _lib.EpsmError(f"the Laplacian table's row {v} is not its degree's worth of neighbours followed by marks")
            out.append(set(kept))
        return out


class AdamUniform(torch.optim.Optimizer):
    """Adam whose second moment is one number per tensor -- the maximum of the element-wise estimate -- instead of one per
    element (Nicolet et al. 2021): every element of a tensor takes a step of the same scale, so the smooth field a
    ``from_differential`` gradient is stays smooth.  ``step``: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
    p -= lr (m / (1 - b1^t)) / sqrt(max(v) / (1 - b2^t)); no epsilon, a tensor whose gradients were all 0 so far does not move."""

    def __init__(self, params, lr: float = 0.1, betas=(0.9, 0.999)):
        super().__init__(params, dict(lr=lr, betas=betas))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if not state:
                    state["step"], state["m"], state["v"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                state["step"] += 1
                t = state["step"]
                state["m"].mul_(b1).add_(p.grad, alpha=1 - b1)
                state["v"].mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                vmax = state["v"].max() / (1 - b2 ** t)
                scale = torch.where(vmax > 0, vmax.sqrt(), torch.ones_like(vmax))
                p.sub_(group["lr"] / (1 - b1 ** t) * state["m"] / scale)
        return loss
