"""Loader of the product library ``libepsm_hip.so`` (C ABI: include/epsm.h).

There is no CPU fallback: if the library is missing or a call fails, an
exception is raised.  ``import torch`` happens first on purpose -- torch-ROCm
ships its own ``libamdhip64.so.7`` and the dynamic loader then binds our
library to that same HIP runtime, so torch streams / device pointers are valid
inside our kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import torch  # loaded before libepsm_hip.so on purpose, see above

from .replays import REPLAYS

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 7          # EPSM_ABI_VERSION of include/epsm.h
LIB_PATH = os.path.join(_HERE, os.environ.get("EPSM_LIB_NAME", "libepsm_hip.so"))   # EPSM_LIB_NAME: A/B builds
_lib = None


class EpsmError(RuntimeError):
    pass


class build_lock:
    """One build of a directory at a time across processes (the ranks of a multi-process run all check their libraries on
    start-up; two `make`s in one directory write the same files, and a third process may dlopen a half-written one)."""

    def __init__(self, directory: str):
        self.path = os.path.join(directory, ".build.lock")

    @staticmethod
    def _open(path: str):
        try:
            return os.open(path, os.O_RDWR | os.O_CREAT, 0o666)
        except OSError:
            return os.open(path, os.O_RDONLY)          # another user's lock file: flock needs no write access

    def __enter__(self):
        import fcntl
        try:
            fd = self._open(self.path)
        except OSError:
            # a built checkout the running user may read but not write: make finds nothing stale and writes nothing,
            # the lock goes to the temporary directory, keyed by the source directory
            import hashlib
            import tempfile
            tag = hashlib.sha256(os.path.dirname(os.path.abspath(self.path)).encode()).hexdigest()[:16]
            fd = self._open(os.path.join(tempfile.gettempdir(), f"epsm_build_{tag}.lock"))
        self.f = os.fdopen(fd, "rb")
        fcntl.flock(self.f, fcntl.LOCK_EX)
        return self

    def __exit__(self, *exc):
        import fcntl
        fcntl.flock(self.f, fcntl.LOCK_UN)
        self.f.close()
        return False


def build(force: bool = False) -> str:
    """Compiles the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    with build_lock(src_dir):
        if force:
            subprocess.run(["make", "-C", src_dir, "-s", "clean"], check=True)
        subprocess.run(["make", "-C", src_dir, "-s"], check=True)
    return LIB_PATH


def _declare(lib):
    lib.epsm_abi_version.restype = C.c_int
    lib.epsm_abi_version.argtypes = []
    lib.epsm_last_error.restype = C.c_char_p
    lib.epsm_last_error.argtypes = []
    lib.epsm_num_param_grads.restype = C.c_int
    lib.epsm_num_param_grads.argtypes = [C.c_int, C.c_int]
    lib.epsm_manifold_grad.restype = C.c_int
    lib.epsm_manifold_grad.argtypes = [
        C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_float,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.epsm_first_vertex_tangent.restype = C.c_int
    lib.epsm_first_vertex_tangent.argtypes = [
        C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.epsm_scatter.restype = C.c_int
    lib.epsm_scatter.argtypes = [
        C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.epsm_manifold_grad_scatter.restype = C.c_int
    lib.epsm_manifold_grad_scatter.argtypes = [
        C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
        C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_float,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.epsm_backward_pass.restype = C.c_int
    lib.epsm_backward_pass.argtypes = [
        C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.epsm_backward_pass_packed.restype = C.c_int
    lib.epsm_backward_pass_packed.argtypes = [
        C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
        C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.epsm_sinkhorn_splits.restype = C.c_int
    lib.epsm_sinkhorn_splits.argtypes = [C.c_int64, C.c_int64]
    lib.epsm_sinkhorn_scratch_bytes.restype = C.c_size_t
    lib.epsm_sinkhorn_scratch_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int]
    lib.epsm_sinkhorn_softmin.restype = C.c_int
    lib.epsm_sinkhorn_softmin.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_sinkhorn_update.restype = C.c_int
    lib.epsm_sinkhorn_update.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_release_workspace.restype = C.c_int
    lib.epsm_release_workspace.argtypes = []
    lib.epsm_set_option.restype = C.c_int
    lib.epsm_set_option.argtypes = [C.c_int, C.c_int64]
    lib.epsm_get_option.restype = C.c_int64
    lib.epsm_get_option.argtypes = [C.c_int]
    lib.epsm_film_adjoint_reparam.restype = C.c_int
    lib.epsm_film_adjoint_reparam.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    lib.epsm_film_splat_tangent.restype = C.c_int
    lib.epsm_film_splat_tangent.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p]
    declare_tracer(lib)
    declare_bvh(lib)
    declare_scene_tables(lib)
    declare_rigid(lib)
    declare_smooth(lib)
    return lib


def declare_rigid(lib):
    """Prototypes of the rigid-motion reduction and its transpose of include/epsm_trace.h (device library only)."""
    lib.epsm_rigid_workspace_bytes.restype = C.c_size_t
    lib.epsm_rigid_workspace_bytes.argtypes = [C.c_int64, C.c_int32]
    lib.epsm_rigid_reduce.restype = C.c_int
    lib.epsm_rigid_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_rigid_expand.restype = C.c_int
    lib.epsm_rigid_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
    return lib


def declare_smooth(lib):
    """Prototypes of the large-steps entry points of include/epsm_trace.h (device library only)."""
    lib.epsm_mesh_laplacian_bytes.restype = C.c_size_t
    lib.epsm_mesh_laplacian_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.epsm_mesh_laplacian.restype = C.c_int
    lib.epsm_mesh_laplacian.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_laplacian_apply.restype = C.c_int
    lib.epsm_laplacian_apply.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.epsm_laplacian_solve_bytes.restype = C.c_size_t
    lib.epsm_laplacian_solve_bytes.argtypes = [C.c_int64]
    lib.epsm_laplacian_solve.restype = C.c_int
    lib.epsm_laplacian_solve.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def declare_bvh(lib):
    """Prototypes of the BVH build / refit of include/epsm_trace.h (device library only)."""
    lib.epsm_bvh_max_nodes.restype = C.c_int64
    lib.epsm_bvh_max_nodes.argtypes = [C.c_int64]
    lib.epsm_bvh_workspace_bytes.restype = C.c_size_t
    lib.epsm_bvh_workspace_bytes.argtypes = [C.c_int64]
    lib.epsm_bvh_build.restype = C.c_int
    lib.epsm_bvh_build.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_bvh_refit.restype = C.c_int
    lib.epsm_bvh_refit.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_int32, C.c_void_p, C.c_void_p]
    return lib


def declare_scene_tables(lib):
    """Prototypes of the device scene tables of include/epsm_trace.h (device library only)."""
    lib.epsm_scene_topology_bytes.restype = C.c_size_t
    lib.epsm_scene_topology_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.epsm_scene_topology_workspace_bytes.restype = C.c_size_t
    lib.epsm_scene_topology_workspace_bytes.argtypes = [C.c_int64]
    lib.epsm_scene_topology.restype = C.c_int
    lib.epsm_scene_topology.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_vertex_normals.restype = C.c_int
    lib.epsm_vertex_normals.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p]
    lib.epsm_vertex_normals_backward_bytes.restype = C.c_size_t
    lib.epsm_vertex_normals_backward_bytes.argtypes = [C.c_int64]
    lib.epsm_vertex_normals_backward.restype = C.c_int
    lib.epsm_vertex_normals_backward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_vertex_normals_forward.restype = C.c_int
    lib.epsm_vertex_normals_forward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.epsm_emitter_tables_bytes.restype = C.c_size_t
    lib.epsm_emitter_tables_bytes.argtypes = [C.c_int64, C.c_int32]
    lib.epsm_emitter_tables.restype = C.c_int
    lib.epsm_emitter_tables.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_environment_tables_bytes.restype = C.c_size_t
    lib.epsm_environment_tables_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.epsm_environment_tables.restype = C.c_int
    lib.epsm_environment_tables.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def declare_tracer(lib):
    """Prototypes of the tracer entry points of include/epsm_trace.h that the HIP library and the host build of the tracer
    (tests/host_harness) both export; tests/_scenes.py applies them to the latter."""
    trace_args = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_uint32]
    lib.epsm_trace_paths.restype = C.c_int
    lib.epsm_trace_paths.argtypes = trace_args + [C.c_void_p]
    lib.epsm_trace_paths_wavefront.restype = C.c_int
    lib.epsm_trace_paths_wavefront.argtypes = trace_args + [C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_trace_paths_color.restype = C.c_int
    lib.epsm_trace_paths_color.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.epsm_trace_workspace_bytes.restype = C.c_size_t
    lib.epsm_trace_workspace_bytes.argtypes = [C.c_int64]
    lib.epsm_trace_reparam_workspace_bytes.restype = C.c_size_t
    lib.epsm_trace_reparam_workspace_bytes.argtypes = [C.c_int64]
    lib.epsm_trace_paths_reparam.restype = C.c_int
    lib.epsm_trace_paths_reparam.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    # scene, seed, path_offset, N, max_depth, rays, kappa, exponent, flags, forward, grad_pos, tan_pos, workspace, bytes, stream
    if hasattr(lib, "epsm_probe_reparam_warps"):           # (the HIP library and tests/host_harness/trace_host.cpp; a host build without it still loads)
        lib.epsm_probe_reparam_warps.restype = C.c_int
        lib.epsm_probe_reparam_warps.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float,
                                                 C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    if hasattr(lib, "epsm_trace_paths_reparam_forward"):   # (the HIP library; of the host builds, tests/host_harness/trace_fwd_host.cpp)
        lib.epsm_trace_reparam_forward_workspace_bytes.restype = C.c_size_t
        lib.epsm_trace_reparam_forward_workspace_bytes.argtypes = [C.c_int64]
        lib.epsm_trace_paths_reparam_forward.restype = C.c_int
        lib.epsm_trace_paths_reparam_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int64,
                                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                         C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                         C.c_void_p]
    # The colour adjoint's replays: scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, then the pass's own.
    # The pass's own comes from the table of replays.py.
    # (hasattr: the HIP library has them all; of the host builds, tests/host_harness/trace_{tex,bsdf,material,alphamap,envpose}_host.cpp)
    replay_args = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    for r in REPLAYS:
        for direction in ("backward", "forward"):
            if hasattr(lib, r.entry(direction)):
                fn = getattr(lib, r.entry(direction))
                fn.restype, fn.argtypes = C.c_int, replay_args + r.tail(direction)
        if r.workspace and hasattr(lib, r.workspace):
            getattr(lib, r.workspace).restype, getattr(lib, r.workspace).argtypes = C.c_size_t, [C.c_int64]
    lib.epsm_film_splat.restype = C.c_int
    lib.epsm_film_splat.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.epsm_film_develop.restype = C.c_int
    lib.epsm_film_develop.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def lib():
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise EpsmError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or make -C epsm_mitsuba3_amd/csrc). There is no CPU fallback.")
        _lib = _declare(C.CDLL(LIB_PATH))
        if _lib.epsm_abi_version() != ABI_VERSION:
            raise EpsmError("libepsm_hip.so ABI version mismatch")
    return _lib


def stream(device):
    """The handle of ``device``'s current stream for the ``void *stream`` argument of the C ABI; None (the null stream) for a
    CPU device, which only the host build of the tracer (tests/host_harness) is called with."""
    device = torch.device(device)
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().epsm_last_error().decode("utf-8", "replace")
        raise EpsmError(f"{what} failed with code {rc}: {msg}")


OPT_SMALL_WAVEFRONT_PATHS, OPT_REPLICAS, OPT_ONE_LAUNCH, OPT_WORKGROUP_SLOTS = 0, 1, 2, 3       # include/epsm.h EPSM_OPT_*
OPT_IOR_GRADS = 5                                                                                # (4 is not assigned)


class options:
    """``with options(small_wavefront_paths=0, replicas=False): ...`` -- launch options of the fused entry points
    (include/epsm.h, epsm_set_option) for the duration of a block; the previous values come back on exit."""

    def __init__(self, small_wavefront_paths=None, replicas=None, one_launch=None, workgroup_slots=None, ior_grads=None):
        self.want = {OPT_SMALL_WAVEFRONT_PATHS: small_wavefront_paths, OPT_REPLICAS: None if replicas is None else int(bool(replicas)),
                     OPT_ONE_LAUNCH: None if one_launch is None else int(bool(one_launch)), OPT_WORKGROUP_SLOTS: workgroup_slots,
                     OPT_IOR_GRADS: None if ior_grads is None else int(bool(ior_grads))}

    def __enter__(self):
        self.saved = {k: lib().epsm_get_option(k) for k, v in self.want.items() if v is not None}
        for k, v in self.want.items():
            if v is not None:
                check(lib().epsm_set_option(k, int(v)), "epsm_set_option")
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            lib().epsm_set_option(k, v)
        return False
