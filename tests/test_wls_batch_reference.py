"""The batch form of the edge-aware disparity filter without a GPU: the interface lists (header, binding, library, ABI version)
and the argument errors of DisparityWLSFilter.filterBatch / StereoSGBM.computeFilteredBatch, all of which are raised before any
engine exists.  What the batch computes is held against tests/wls_ref.py on the device: tests/test_gpu_wls_batch.py."""
import os
import re

import numpy as np
import pytest

import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_wls_filter_batch", "sgm_wls_filter_batch_device"]


def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_wls_batch.h")).read()
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", extra, flags=re.S))))
    assert declared == sorted(_lib.WLS_BATCH_EXPORTS) == NEW
    assert '#include "sgm_hip_wls_batch.h"' in txt and all(hasattr(_lib.load(), n) for n in declared)
    for other in (_lib.EXPORTS, _lib.CONFIDENCE_EXPORTS, _lib.RIGHT_EXPORTS, _lib.WLS_EXPORTS):
        assert not set(_lib.WLS_BATCH_EXPORTS) & set(other)
    assert sorted(_lib.WLS_EXPORTS) == ["sgm_wls_filter", "sgm_wls_filter_device", "sgm_wls_weights"]
    assert _lib.load().sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt)
    assert all(callable(getattr(cv.Engine, n)) for n in ("wls_filter_batch_host", "wls_filter_batch_device"))
    assert callable(cv.DisparityWLSFilter.filterBatch) and callable(cv.StereoSGBM.computeFilteredBatch)


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU; so are N <= 0 and a bad channel count"""
    L = _lib.load()
    lut = cv.wls_weights(1.5)
    one = (np.ctypeslib.ctypes.c_void_p * 1)(8)
    for fn in (L.sgm_wls_filter_batch, L.sgm_wls_filter_batch_device):
        assert fn(None, 1, one, one, 1, None, 4, 4, -16, 8000.0, lut.ctypes.data, one, None) == -1      # SGM_ERR_INVALID_ARG
        assert b"sgm_wls_filter" in L.sgm_last_error()
        assert fn(None, 0, one, one, 1, None, 4, 4, -16, 8000.0, lut.ctypes.data, one, None) == -1
        assert b"N=0" in L.sgm_last_error()


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_filter_batch_argument_errors_come_before_any_engine(no_engine):
    f = cv.createDisparityWLSFilter()
    d, g, c = np.zeros((2, 6, 9), np.int16), np.zeros((2, 6, 9), np.uint8), np.zeros((2, 6, 9), np.uint8)
    g3 = np.zeros((2, 6, 9, 3), np.uint8)
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(d, g[:, :, :8])
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(d, g, c[:, :5])
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(d, g[:1])                                         # one guide for two maps
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(d, g3, c[:1])
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch([d[0], d[1]], [g[0], g[1, :5]])                   # a sequence whose maps differ in shape
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(d, np.zeros((2, 9, 6, 3), np.uint8))
    with pytest.raises(cv.error, match="CV_16SC1"):
        f.filterBatch(d.astype(np.int32), g)
    with pytest.raises(cv.error, match="CV_8U"):
        f.filterBatch(d, g.astype(np.float32))
    with pytest.raises(cv.error, match="CV_8UC1"):
        f.filterBatch(d, g, c.astype(np.int16))
    with pytest.raises(cv.error, match="CV_16SC1"):
        f.filterBatch([d[0], d[1].astype(np.int32)], g)
    for gbad in (np.zeros((2, 6, 9, 2), np.uint8), np.zeros((2, 6, 9, 4), np.uint8), np.zeros((2, 6, 9, 3, 1), np.uint8), np.zeros((2, 54), np.uint8)):
        with pytest.raises(cv.error, match=r"\(N, H, W\) or \(N, H, W, 3\)"):
            f.filterBatch(d, gbad)
    with pytest.raises(cv.error, match=r"\(N, H, W\)"):
        f.filterBatch(d[0], g[0])                                       # a single map is not a batch
    with pytest.raises(cv.error, match=r"\(N, H, W\)"):
        f.filterBatch(np.zeros((2, 6, 9, 1), np.int16), g)
    with pytest.raises(cv.error, match="empty"):
        f.filterBatch(np.zeros((0, 6, 9), np.int16), np.zeros((0, 6, 9), np.uint8))
    with pytest.raises(cv.error, match="empty"):
        f.filterBatch([], [])
    with pytest.raises(cv.error, match="empty"):
        f.filterBatch(np.zeros((2, 0, 9), np.int16), np.zeros((2, 0, 9), np.uint8))
    with pytest.raises(cv.error, match="empty"):
        f.filterBatch(np.zeros((2, 6, 0), np.int16), np.zeros((2, 6, 0, 3), np.uint8))
    with pytest.raises(cv.error, match="outside int16"):
        f.filterBatch(d, g, invalid=40000)
    # mixed host / device inputs: a torch tensor that is not on the GPU beside numpy, as a stack and inside a sequence
    import torch
    with pytest.raises(cv.error, match="CUDA"):
        f.filterBatch(torch.from_numpy(d), g)
    with pytest.raises(cv.error, match="CUDA"):
        f.filterBatch([d[0], d[1]], [g[0], torch.from_numpy(g[1])])
    with pytest.raises(cv.error, match="CUDA"):
        f.filterBatch(d, g, torch.from_numpy(c))


def test_compute_filtered_batch_argument_errors_come_before_any_engine(no_engine):
    m = cv.StereoSGBM_create(numDisparities=16)
    l = np.zeros((2, 6, 40), np.uint8)
    with pytest.raises(cv.error, match="the same number"):
        m.computeFilteredBatch(l, l[:1])
    with pytest.raises(cv.error, match="the same number"):
        m.computeFilteredBatch([], [])
    with pytest.raises(cv.error, match="left.size\\(\\) == right.size\\(\\)"):
        m.computeFilteredBatch(l, l[:, :, :39])
    with pytest.raises(cv.error, match="CV_8U"):
        m.computeFilteredBatch(l.astype(np.int16), l.astype(np.int16))
    with pytest.raises(cv.error, match="CV_8U"):
        m.computeFilteredBatch([l[0], l[1]], [l[0], l[1].astype(np.float32)])
    with pytest.raises(cv.error, match="channels"):
        m.computeFilteredBatch(np.zeros((2, 6, 40, 2), np.uint8), np.zeros((2, 6, 40, 2), np.uint8))
    with pytest.raises(cv.error, match="channels"):
        m.computeFilteredBatch(l[0], l[0])                              # a single pair is not a batch
    with pytest.raises(cv.error, match="empty"):
        m.computeFilteredBatch(np.zeros((2, 0, 40), np.uint8), np.zeros((2, 0, 40), np.uint8))
    with pytest.raises(cv.error, match="width < 2"):
        m.computeFilteredBatch(np.zeros((2, 6, 1), np.uint8), np.zeros((2, 6, 1), np.uint8))
    with pytest.raises(cv.error, match="setLambda"):
        m.computeFilteredBatch(l, l, lambda_=-1.0)
    with pytest.raises(cv.error, match="setSigmaColor"):
        m.computeFilteredBatch(l, l, sigmaColor=0.0)
    with pytest.raises(cv.error, match="MODE_SGBM_3WAY"):
        cv.StereoSGBM_create(numDisparities=16, mode=cv.STEREO_SGBM_MODE_SGBM_3WAY).computeFilteredBatch(l, l)
    import torch
    with pytest.raises(cv.error, match="CUDA"):
        m.computeFilteredBatch(torch.from_numpy(l), l)
    with pytest.raises(cv.error, match="colour census"):
        cv.StereoSGBM_create(numDisparities=16, costFunction=cv.STEREO_COST_CENSUS).computeFilteredBatch(
            np.zeros((2, 6, 40, 3), np.uint8), np.zeros((2, 6, 40, 3), np.uint8))
