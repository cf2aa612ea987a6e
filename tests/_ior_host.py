"""The host build of the constraint-parallel core with the eta column (tests/host_harness/cp_ior_host.cpp: cp_core_host.cpp plus
geta = d / d eta_k per (vertex, path); test infrastructure).  Built into its own library with the flags the host harness's
Makefile gives libcp_core_host.so -- under EPSM_SAN=1 with its sanitizer flags, `_san` suffix; into a per-user temporary
directory when the checkout is read-only."""
import ctypes as C
import glob
import hashlib
import os
import subprocess
import tempfile

import torch

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_harness")
_SRC = os.path.join(_DIR, "cp_ior_host.cpp")
_lib = None
_SAN = os.environ.get("EPSM_SAN", "0") == "1"
_NAME = "libcp_ior_host_san.so" if _SAN else "libcp_ior_host.so"


def _sources():
    root = os.path.dirname(os.path.dirname(_DIR))
    return ([_SRC, os.path.join(_DIR, "cp_core_host.cpp")]
            + glob.glob(os.path.join(root, "epsm_mitsuba3_amd", "csrc", "*.h")) + glob.glob(os.path.join(root, "include", "*.h")))


def _stale(so):
    return not os.path.isfile(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in _sources())


def build_host_ior() -> str:
    from epsm_mitsuba3_amd._lib import build_lock
    so = os.path.join(_DIR, _NAME)
    if not os.access(_DIR, os.W_OK) and _stale(so):
        tag = hashlib.sha256(_DIR.encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), f"epsm_ior_host_{os.getuid()}_{tag}")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, _NAME)
    with build_lock(os.path.dirname(so)):
        if _stale(so):
            opt = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if _SAN else ["-O2"]
            cmd = [os.environ.get("CXX", "g++")] + opt + ["-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off",
                   "-o", so + ".tmp", _SRC]
            subprocess.run(cmd, check=True)
            os.replace(so + ".tmp", so)
    return so


def host_ior_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_host_ior())
        for name in ("epsm_host_cp_ior_f32", "epsm_host_cp_ior_f64"):
            fn = getattr(_lib, name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_double,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def host_ior_calc_grad(variant, path_info, dlduv, dldp, clip=0.1, dtype=torch.float64, dlduv_cols=None):
    """-> (param list, light list, diffuse list, geta (K,N)) of the host build of epsm_cp_core.h: calc_grad's dense lists as
    host_core.host_core_calc_grad(core="cp") returns them, and d / d eta_k after the same clamp / NaN rule."""
    from epsm_mitsuba3_amd.records import PackedRecords, VARIANTS, num_param_grads
    rec = PackedRecords(path_info, device="cpu", float_dtype=dtype)
    N, K = rec.N, rec.K
    d = dlduv.detach().to("cpu", dtype).reshape(N, -1).contiguous()
    p = dldp.detach().to("cpu", dtype).reshape(N, 3).contiguous()
    if dlduv_cols is None:
        nzc = torch.nonzero((d != 0).any(dim=0)).flatten()
        dlduv_cols = int(nzc.max()) + 1 if nzc.numel() else 0
        dlduv_cols = max(2, dlduv_cols + (dlduv_cols & 1))
    P = num_param_grads(variant, K)
    out_p = torch.full((P, N, 3), float("nan"), dtype=dtype)
    out_l = torch.full((K, N, 3), float("nan"), dtype=dtype)
    out_d = torch.full((K, N, 3), float("nan"), dtype=dtype)
    geta = torch.full((K, N), float("nan"), dtype=dtype)
    fn = getattr(host_ior_lib(), "epsm_host_cp_ior" + ("_f32" if dtype == torch.float32 else "_f64"))
    rc = fn(VARIANTS[variant], N, K, rec.cam.data_ptr(), C.addressof(rec.records), d.data_ptr(), d.shape[1], dlduv_cols, p.data_ptr(),
            float(clip), out_p.data_ptr(), out_l.data_ptr(), out_d.data_ptr(), geta.data_ptr())
    assert rc == 0
    return list(out_p.unbind(0)), list(out_l.unbind(0)), list(out_d.unbind(0)), geta


def ior_row_values(eta, geta, gm, dhf):
    """The scalar row of every (vertex, path) under EPSM_OPT_IOR_GRADS (csrc/epsm_backward_cp.hip, Emitter::vertex):
    ``eta != 1 ? fin(geta) * dhf.x : dot(fin(gm), dhf)`` -- eta, geta (K,N); gm, dhf (K,N,3), clamped already; -> (K,N) float64."""
    eta, geta, gm, dhf = (t.double() for t in (eta, geta, gm, dhf))
    return torch.where(eta != 1.0, geta * dhf[..., 0], (gm * dhf).sum(dim=-1))


def ior_alpha_buffer(variant, path_info, scatter_info, dlduv, dldp, B, clip=0.1, dtype=torch.float64, keep=None):
    """-> (alpha (B,) float64, refracted (B,) bool): the ``alpha`` buffer the backward pass owes under EPSM_OPT_IOR_GRADS -- the
    float64 sum over the host core's outputs of ``ior_row_values`` -- and the slots that receive a vertex with eta != 1.
    ``path_info`` / ``scatter_info`` on the CPU; the alpha slot of a vertex is aux[0]; ``keep`` (N,) bool: only these paths."""
    K = len(path_info) - 1
    fp, _, _, geta = host_ior_calc_grad(variant, path_info, dlduv, dldp, clip=clip, dtype=dtype)
    N = geta.shape[1]
    alpha = torch.zeros(B, dtype=torch.float64)
    refracted = torch.zeros(B, dtype=torch.bool)
    for k in range(1, K + 1):
        aux = scatter_info[k - 1].get("aux")
        if aux is None:
            continue
        aux = aux.cpu()
        bid = aux[:, 0].long()
        dhf = aux[:, 1:4].contiguous().view(torch.float32).double()
        gm = fp[5 * (k - 1) + 4].double() if 5 * (k - 1) + 4 < len(fp) else torch.zeros((N, 3), dtype=torch.float64)
        eta = path_info[k]["eta"].cpu().float()
        val = ior_row_values(eta[None], geta[k - 1][None], gm[None], dhf[None])[0]
        ok = (bid >= 0) & (bid < B)
        if keep is not None:
            ok &= keep.cpu().bool()
        alpha.index_add_(0, bid[ok], val[ok])
        refracted[bid[ok & (eta != 1.0) & (path_info[k]["active"].cpu() != 0) & (path_info[k]["ismesh"].cpu() > 0)]] = True       # (a dead vertex, or one that left the scene, logs zeros: eta = 0 on slot 0)
    return alpha, refracted


if __name__ == "__main__":          # __graft_entry__.build()
    build_host_ior()
