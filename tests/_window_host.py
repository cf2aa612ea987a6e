"""The host build of the backward kernel's window bookkeeping (tests/host_harness/cp_window_host.cpp: the slot word and the
window schedule of epsm_cp_core.h) -- test infrastructure.  Built into its own library with the flags the host harness's
Makefile gives libcp_core_host.so -- under EPSM_SAN=1 (tools/run_san.sh) with its sanitizer flags, `_san` suffix; into a
per-user temporary directory when the checkout is read-only."""
import ctypes as C
import glob
import hashlib
import os
import subprocess
import tempfile

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_harness")
_SRC = os.path.join(_DIR, "cp_window_host.cpp")
_lib = None
_SAN = os.environ.get("EPSM_SAN", "0") == "1"
_NAME = "libcp_window_host_san.so" if _SAN else "libcp_window_host.so"
FIELDS = ["nv", "idstar"] + [f"a{k}" for k in range(1, 6)] + [f"b{k}" for k in range(1, 6)] + ["diffuse1", "active1", "in_range", "slot"]


def _sources():
    root = os.path.dirname(os.path.dirname(_DIR))
    return [_SRC] + glob.glob(os.path.join(root, "epsm_mitsuba3_amd", "csrc", "*.h")) + glob.glob(os.path.join(root, "include", "*.h"))


def _stale(so):
    return not os.path.isfile(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in _sources())


def build_host_window() -> str:
    from epsm_mitsuba3_amd._lib import build_lock
    so = os.path.join(_DIR, _NAME)
    if not os.access(_DIR, os.W_OK) and _stale(so):
        tag = hashlib.sha256(_DIR.encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), f"epsm_window_host_{os.getuid()}_{tag}")
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


def host_window():
    global _lib
    if _lib is None:
        lib = C.CDLL(build_host_window())
        lib.epsm_host_slot_words.restype = None
        lib.epsm_host_slot_words.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32] + [C.c_void_p] * 4
        lib.epsm_host_window_count.restype = C.c_int64
        lib.epsm_host_window_count.argtypes = [C.c_int64, C.c_int64, C.c_int]
        lib.epsm_host_windows.restype = None
        lib.epsm_host_windows.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        lib.epsm_host_windows_per_workgroup.restype = C.c_int64
        lib.epsm_host_windows_per_workgroup.argtypes = [C.c_int64, C.c_int64]
        _lib = lib
    return _lib


def slot_words(variant, K, fw, in_range, slot):
    """-> (plan, word, fields_plan, fields_word) of the flag words `fw` (uint32 array) at window slot `slot`; fields: FIELDS."""
    import numpy as np
    fw = np.ascontiguousarray(fw, dtype=np.uint32)
    inr = np.ascontiguousarray(in_range, dtype=np.uint8)
    n = fw.shape[0]
    plan, word = np.empty(n, np.uint32), np.empty(n, np.uint32)
    fp, fs = np.empty((n, len(FIELDS)), np.int32), np.empty((n, len(FIELDS)), np.int32)
    host_window().epsm_host_slot_words(variant, K, fw.ctypes.data, inr.ctypes.data, n, slot, plan.ctypes.data, word.ctypes.data,
                                       fp.ctypes.data, fs.ctypes.data)
    return plan, word, fp, fs


def windows(n, S, W):
    """-> (first, size) of every window of n paths with S workgroup slots and bulk windows of W, and the launcher's count."""
    import numpy as np
    lib = host_window()
    count = lib.epsm_host_window_count(n, S, W)
    first, size = np.empty(count, np.int64), np.empty(count, np.int32)
    lib.epsm_host_windows(n, S, W, 0, count, first.ctypes.data, size.ctypes.data)
    return first, size, count


if __name__ == "__main__":          # __graft_entry__.build()
    build_host_window()
