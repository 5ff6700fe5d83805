"""ctypes front end of the volume-form oracle (sgbm_volume_oracle.h) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Stands beside oracle.py, which stays as it is (bench.py imports it): the frozen oracle refuses MODE_HH4 and colour pairs,
this one takes modes 0, 1, 3 on 1 or 3 channels and returns the same taps.  Only tests/ and tools/ load it.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from .oracle import Params, Taps, make_params

_HERE = os.path.dirname(os.path.abspath(__file__))
# ORACLE_SANITIZE=1: the AddressSanitizer + UBSan build (tools/sanitize_oracle.sh), as oracle.py
_ASAN = os.environ.get("ORACLE_SANITIZE") == "1"
_SO = os.path.join(_HERE, "liboracle_volume_asan.so" if _ASAN else "liboracle_volume.so")


def build(force: bool = False) -> str:
    src = [os.path.join(_HERE, f) for f in ("sgbm_volume_oracle.c", "sgbm_volume_oracle.h", "sgbm_oracle.c", "sgbm_oracle.h")]
    stale = (not os.path.exists(_SO)) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in src)
    if force or stale:
        subprocess.run(["make", "-C", _HERE, "-B" if force else "-s", os.path.basename(_SO)], check=True, capture_output=True)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_SO)
        L.volume_oracle_compute.restype = C.c_int
        L.volume_oracle_compute.argtypes = [C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                            C.c_void_p, C.POINTER(Taps)]
        _lib = L
    return _lib


def geometry(p: Params, W: int):
    """(minX1, W1) -- SURVEY.md A.1, stated here so that this module needs nothing of the frozen library"""
    maxD = p.minDisparity + p.numDisparities
    minX1 = max(maxD, 0)
    return minX1, W + min(p.minDisparity, 0) - minX1


def sgbm_compute(left: np.ndarray, right: np.ndarray, taps=False, **kw):
    """The map of a gray (H, W) or colour (H, W, 3) uint8 pair, modes 0, 1 and 3.  taps as oracle.sgbm_compute: True adds a
    dict with C, S, disp_raw, disp_median and the headroom record, "light" leaves the two volumes out."""
    p = kw.pop("params", None) or make_params(**kw)
    left = np.ascontiguousarray(left, dtype=np.uint8)
    right = np.ascontiguousarray(right, dtype=np.uint8)
    assert left.shape == right.shape and (left.ndim == 2 or (left.ndim == 3 and left.shape[2] == 3)), left.shape
    H, W = left.shape[:2]
    cn = 1 if left.ndim == 2 else 3
    disp = np.empty((H, W), np.int16)
    t = Taps()
    out = {}
    if taps:
        _, W1 = geometry(p, W)
        if W1 > 0 and taps != "light":
            out["C"] = np.zeros((H, W1, p.numDisparities), np.int16)
            out["S"] = np.zeros((H, W1, p.numDisparities), np.int16)
            t.C = out["C"].ctypes.data
            t.S = out["S"].ctypes.data
        out["disp_raw"] = np.empty((H, W), np.int16)
        out["disp_median"] = np.empty((H, W), np.int16)
        t.disp_raw = out["disp_raw"].ctypes.data
        t.disp_median = out["disp_median"].ctypes.data
    rc = lib().volume_oracle_compute(C.byref(p), left.ctypes.data, right.ctypes.data, H, W, cn, left.strides[0],
                                     disp.ctypes.data, C.byref(t))
    if rc != 0:
        raise ValueError(f"volume_oracle_compute failed rc={rc}")
    if taps:
        out.update(max_cost_plus_p2=t.max_cost_plus_p2, max_delta=t.max_delta, headroom_ok=bool(t.headroom_ok))
        return disp, out
    return disp
