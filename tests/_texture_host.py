"""The host build of the texel adjoint (tests/host_harness/trace_tex_host.cpp: trace_host.cpp, the reparameterised forward pass of
trace_fwd_host.cpp, and epsm_trace_paths_texture_backward / _forward) as a Scene backend (test infrastructure).  Built into its own
library with the flags the host harness's Makefile gives libtrace_host.so; into a per-user temporary directory when the checkout
is read-only."""
import ctypes as C
import glob
import hashlib
import os
import subprocess
import tempfile

from _scenes import _DIR

_SRC = os.path.join(_DIR, "trace_tex_host.cpp")
_lib = None


def _sources():
    root = os.path.dirname(os.path.dirname(_DIR))
    return ([_SRC, os.path.join(_DIR, "trace_fwd_host.cpp"), os.path.join(_DIR, "trace_host.cpp")]
            + glob.glob(os.path.join(root, "epsm_mitsuba3_amd", "csrc", "*.h")) + glob.glob(os.path.join(root, "include", "*.h")))


def _stale(so):
    return not os.path.isfile(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in _sources())


def build_host_texture() -> str:
    from epsm_mitsuba3_amd._lib import build_lock
    so = os.path.join(_DIR, "libtrace_tex_host.so")
    if not os.access(_DIR, os.W_OK) and _stale(so):
        tag = hashlib.sha256(_DIR.encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), f"epsm_tex_host_{os.getuid()}_{tag}")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, "libtrace_tex_host.so")
    with build_lock(os.path.dirname(so)):
        if _stale(so):
            cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off",
                   "-fopenmp", "-o", so + ".tmp", _SRC]
            subprocess.run(cmd, check=True)
            os.replace(so + ".tmp", so)
    return so


def host_texture_tracer():
    global _lib
    if _lib is None:
        from epsm_mitsuba3_amd._lib import declare_tracer
        _lib = declare_tracer(C.CDLL(build_host_texture()))
    return _lib


def on_host_texture(scene):
    scene._backend = host_texture_tracer()
    return scene


if __name__ == "__main__":          # __graft_entry__.build()
    build_host_texture()
