"""The trace builds' time log on a box without a GPU: tests/emu's host-compiled device code with the list form of
madsim_hip_timeline_seeds as one more entry point (tests/span_emu/emu_timeline.cpp).  Test-only, never imported by madsim_amd/."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

from madsim_amd import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = os.path.join(_HERE, "libmadsim_emu_timeline.so")
_SRCS = [os.path.join(_HERE, "emu_timeline.cpp"), os.path.join(_ROOT, "tests", "emu", "emu_driver.cpp"), os.path.join(_ROOT, "tests", "emu", "emu_shim.h"),
         os.path.join(_ROOT, "madsim_amd", "csrc", "sim_kernel.h"), os.path.join(_ROOT, "madsim_amd", "csrc", "geometry.h"),
         *sorted(glob.glob(os.path.join(_ROOT, "madsim_amd", "csrc", "kernel", "*.h"))), os.path.join(_ROOT, "include", "madsim_hip.h")]


def _stale():
    return not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in _SRCS)


def build():
    """(pytest-xdist workers may arrive together: one builds under a file lock into a temporary name, the others wait)"""
    if _stale():
        import fcntl
        with open(_LIB + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if _stale():
                tmp = f"{_LIB}.{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DMADSIM_EMU", "-x", "c++",
                                       "-I" + os.path.join(_ROOT, "tests", "emu"), "-o", tmp, _SRCS[0]])
                os.replace(tmp, _LIB)
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.madsim_emu_timeline_seeds.argtypes = [C.POINTER(A.Workload), C.POINTER(A.Config), C.c_void_p, C.c_uint64, C.POINTER(A.Limits), C.c_void_p,
                                                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.madsim_emu_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def timeline(workload, seeds, obs_cap=256, config=None, limits=None, times=True):
    """(results ndarray[A.RESULT_DTYPE], values uint64[n, obs_cap], times uint64[n, obs_cap], true lengths uint64[n], feature mask of the
    trace build that ran) of the listed seeds, as madsim_hip_timeline_seeds gives them; times=False passes no time log (the time array
    comes back as it was allocated: zeros)."""
    cfg, lim = config or A.Config.default(), limits or A.Limits()
    s = np.array([int(x) for x in seeds], dtype=np.uint64)
    n = len(s)
    out, lens = np.zeros(n, dtype=A.RESULT_DTYPE), np.zeros(n, dtype=np.uint64)
    both = np.zeros((2, n, obs_cap), dtype=np.uint64)          # one allocation, as the library lays them out: the time rows behind the observation rows
    obs, tim = both[0], both[1]
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    rc = lib().madsim_emu_timeline_seeds(workload.ref(), C.byref(cfg), p(s), n, C.byref(lim), p(obs), p(tim) if times else None, obs_cap, p(lens), p(out))
    if rc < 0:
        raise RuntimeError(f"emu error {rc}: {lib().madsim_emu_last_error().decode()}")
    return out, obs, tim, lens, rc
