"""Synthetic wavefronts for the tests of EPSM_OPT_IOR_GRADS (test_ior_synthetic.py on the CPU, test_gpu_ior_backward.py on the
device): seeded records of ``SyntheticScene`` built on the CPU, and the ``alpha`` buffer the backward pass owes for them -- the
float64 sum over the host core's outputs of the per-vertex rule (tests/_ior_host.py, ior_alpha_buffer) -- with the allowance of
test_gpu_pipeline.py's yardstick: the weight of the components within 2 % of the clamp plus twice the float32 core's distance
from the float64 one.  Test infrastructure; every case is built once per process and left unchanged."""
import functools

import torch

RES, SPP, V, B = 32, 9, 3000, 4          # 32 x 32 x 9 = 9 216 paths hold every N below
N_RAGGED, N_REPLICAS, N_LARGE = 200, 8192 + 37, 2 * 2048 + 300
PROFILES = [("manifold", "pool"), ("manifold", "mixed"), ("manifold_caustic", "pool")]
KS = [1, 3, 5]
QUIET_SLOT = 0                           # the vertices of this slot are made reflections: its entry must not change with the option


@functools.lru_cache(maxsize=None)
def case(variant, profile, K, N):
    """-> dict(trace (CPU PathTrace of N paths), grad_in (RES,RES,5), dlduv, dldp (float64, the oracle's first-vertex tangent))"""
    import epsm_mitsuba3_amd as epsm
    from oracle.binding import oracle_first_vertex_tangent
    scene = epsm.SyntheticScene(res=RES, n_vertices=K, n_scene_vertices=V, n_bsdfs=B, profile=profile, device="cpu")
    tr = scene.tile(0, 0, N, 17 + K, SPP, K)
    for k in range(1, K + 1):
        tr.path_info[k]["eta"][tr.scatter_info[k - 1]["aux"][:, 0] == QUIET_SLOT] = 1.0
    g = torch.Generator().manual_seed(29)
    grad_in = torch.randn((RES, RES, 5), generator=g) * 2e-5
    first = tr.path_info[1]
    dlduv, dldp, _ = oracle_first_vertex_tangent(tr.ray_o, tr.ray_d, tr.ray_dx, tr.ray_dy, grad_in, SPP, RES, first["points"][0],
                                                 first["points"][1], first["points"][2], first["active"], 2, 0)
    return {"trace": tr, "grad_in": grad_in, "dlduv": dlduv.double(), "dldp": dldp.double(), "variant": variant, "K": K, "N": N}


@functools.lru_cache(maxsize=None)
def private_case(variant, profile, K, N):
    """The records of ``case`` with PRIVATE addressing (tests/_per_path.py): every (path, vertex) has its own triangle rows and its
    own alpha slot, so every entry of the buffers is ONE term -- its bits are the arithmetic's, not the order of the float atomics
    that add the terms of a shared row (which no two launches of the accumulating kernel repeat).  -> dict like ``case`` plus
    V, B and ``reflections`` (B,) bool: the slots whose vertex has eta == 1."""
    import copy
    from _per_path import private_addressing
    c = dict(case(variant, profile, K, N))
    tr = copy.copy(c["trace"])
    _, si = private_addressing(N, K, "cpu", torch.Generator().manual_seed(31 + K))
    tr.scatter_info = si
    c["trace"], c["V"], c["B"] = tr, 6 * N * K, N * K
    c["reflections"] = torch.cat([tr.path_info[k]["eta"].float() == 1.0 for k in range(1, K + 1)])
    return c


def list_keep(N):
    """about an eighth of the paths"""
    return torch.arange(N) % 8 == 3


@functools.lru_cache(maxsize=None)
def reference(variant, profile, K, N, listed=False):
    """-> (alpha (B,) float64, allowance (B,), refracted (B,) bool, alpha without the option (B,)) for the whole wavefront or,
    ``listed``, for the paths of ``list_keep`` alone"""
    from _ior_host import ior_alpha_buffer
    c = case(variant, profile, K, N)
    tr = c["trace"]
    keep = list_keep(N) if listed else None
    run = lambda clip, dtype: ior_alpha_buffer(variant, tr.path_info, tr.scatter_info, c["dlduv"], c["dldp"], B, clip=clip, dtype=dtype, keep=keep)
    alpha, refracted = run(0.1, torch.float64)
    lo, hi, f32 = run(0.098, torch.float64)[0], run(0.102, torch.float64)[0], run(0.1, torch.float32)[0]
    allow = (lo - hi).abs() + 2 * (f32 - alpha).abs()
    return alpha, allow, refracted, plain_alpha(variant, profile, K, N, listed)


def plain_alpha(variant, profile, K, N, listed=False):
    """what the same wavefront gives WITHOUT the option: aux[1..3] . clamp(d / d m_k) on every vertex"""
    from host_core import host_core_calc_grad
    c = case(variant, profile, K, N)
    tr = c["trace"]
    fp, _, _ = host_core_calc_grad(variant, tr.path_info, c["dlduv"], c["dldp"], dtype=torch.float64, core="cp")
    out = torch.zeros(B, dtype=torch.float64)
    keep = list_keep(N) if listed else torch.ones(N, dtype=torch.bool)
    for k in range(1, K + 1):
        if 5 * (k - 1) + 4 >= len(fp):
            continue
        aux = tr.scatter_info[k - 1]["aux"]
        bid = aux[:, 0].long()
        ok = (bid >= 0) & (bid < B) & keep
        val = (fp[5 * (k - 1) + 4].double() * aux[:, 1:4].contiguous().view(torch.float32).double()).sum(dim=1)
        out.index_add_(0, bid[ok], val[ok])
    return out
