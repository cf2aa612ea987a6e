"""The host build of the envmap pose adjoint (tests/host_harness/trace_envpose_host.cpp: trace_material_host.cpp and all it
includes, plus epsm_trace_paths_envpose_backward / _forward and the test-only item export) as a Scene backend (test infrastructure).  Built into its own library with the flags
the host harness's Makefile gives libtrace_host.so -- under EPSM_SAN=1 (tools/run_san.sh) with its sanitizer flags, `_san`
suffix; into a per-user temporary directory when the checkout is read-only."""
import ctypes as C
import glob
import hashlib
import os
import subprocess
import tempfile

from _scenes import _DIR

_SRC = os.path.join(_DIR, "trace_envpose_host.cpp")
_lib = None
_SAN = os.environ.get("EPSM_SAN", "0") == "1"
_NAME = "libtrace_envpose_host_san.so" if _SAN else "libtrace_envpose_host.so"


def _sources():
    root = os.path.dirname(os.path.dirname(_DIR))
    return ([_SRC, os.path.join(_DIR, "trace_material_host.cpp"), os.path.join(_DIR, "trace_bsdf_host.cpp"), os.path.join(_DIR, "trace_tex_host.cpp"), os.path.join(_DIR, "trace_fwd_host.cpp"), os.path.join(_DIR, "trace_host.cpp")]
            + glob.glob(os.path.join(root, "epsm_mitsuba3_amd", "csrc", "*.h")) + glob.glob(os.path.join(root, "include", "*.h")))


def _stale(so):
    return not os.path.isfile(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in _sources())


def build_host_envpose() -> str:
    from epsm_mitsuba3_amd._lib import build_lock
    so = os.path.join(_DIR, _NAME)
    if not os.access(_DIR, os.W_OK) and _stale(so):
        tag = hashlib.sha256(_DIR.encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), f"epsm_envpose_host_{os.getuid()}_{tag}")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, _NAME)
    with build_lock(os.path.dirname(so)):
        if _stale(so):
            opt = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if _SAN else ["-O2"]
            cmd = [os.environ.get("CXX", "g++")] + opt + ["-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off",
                   "-fopenmp", "-o", so + ".tmp", _SRC]
            subprocess.run(cmd, check=True)
            os.replace(so + ".tmp", so)
    return so


def host_envpose_tracer():
    global _lib
    if _lib is None:
        from epsm_mitsuba3_amd._lib import declare_tracer
        _lib = declare_tracer(C.CDLL(build_host_envpose()))
    return _lib


def on_host_envpose(scene):
    scene._backend = host_envpose_tracer()
    return scene


if __name__ == "__main__":          # __graft_entry__.build()
    build_host_envpose()
