"""The left-right consistency confidence without a GPU: hand-worked answers of the definition (include/sgm_hip_lrc.h) held
against its numpy restatement tests/lrc_ref.py, the condition on the generated inputs that keeps the device tests from passing
on maps of zeros, the interface lists (header, binding, library, ABI version), and the Python argument errors, all of which are
raised before any engine exists.  What the device computes is held against lrc_ref.py in tests/test_gpu_lrc.py."""
import os
import re

import numpy as np
import pytest

import lrc_ref as LR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_lrc_confidence", "sgm_lrc_confidence_batch_device", "sgm_lrc_confidence_device"]
INV = -16


def i16(x):
    return np.asarray(x, np.int16)


# ---- the definition, by hand ---------------------------------------------------------------------------------------------------
def test_smoothness_of_a_1x5_map_by_hand():
    """r = 1, V = 2304, M = 0 16 32 . 48 (the dot invalid).  F = 100 - min(100, 100 num / (n^2 V)), num = n s2 - s1^2"""
    M = i16([[0, 16, 32, INV, 48]])
    # p0: {0, 16}      n = 2, s1 = 16, s2 = 256,  num = 512 - 256 = 256,    25600 / 9216 = 2
    # p1: {0, 16, 32}  n = 3, s1 = 48, s2 = 1280, num = 3840 - 2304 = 1536, 153600 / 20736 = 7
    # p2: {16, 32}     n = 2, s1 = 48, s2 = 1280, num = 2560 - 2304 = 256,  25600 / 9216 = 2
    # p3: invalid -> 0;   p4: {48}  n = 1, num = 0 -> 100
    assert 25600 // (4 * 2304) == 2 and 153600 // (9 * 2304) == 7
    assert LR.smoothness(M, INV, 1, 2304).tolist() == [[98, 93, 98, 0, 100]]
    # V = 64: p0 25600 / 256 = 100 -> 0; p1 153600 / 576 = 266 -> capped at 100 -> 0
    assert LR.smoothness(M, INV, 1, 64).tolist() == [[0, 0, 0, 0, 100]]


def test_smoothness_of_a_3x3_map_by_hand():
    """r = 1, V = 2304, one 48 in the middle of zeros: s1 = 48, s2 = 2304 wherever the window holds the middle"""
    M = np.zeros((3, 3), np.int16)
    M[1, 1] = 48
    # corner: n = 4, num = 4 * 2304 - 2304 = 6912,  691200 / 36864 = 18
    # edge:   n = 6, num = 6 * 2304 - 2304 = 11520, 1152000 / 82944 = 13
    # middle: n = 9, num = 9 * 2304 - 2304 = 18432, 1843200 / 186624 = 9
    assert (691200 // 36864, 1152000 // 82944, 1843200 // 186624) == (18, 13, 9)
    assert LR.smoothness(M, INV, 1, 2304).tolist() == [[82, 87, 82], [87, 91, 87], [82, 87, 82]]


def test_radius_zero_gives_full_smoothness_on_every_valid_pixel():
    s = LR.random_pair(20, 40, 3)
    for M in (s["dl"], s["dr"]):
        F = LR.smoothness(M, INV, 0, 1)
        assert np.array_equal(F, np.where(M != INV, 100, 0))


def test_a_constant_pair_is_fully_confident_wherever_the_match_stays_inside():
    H, W, d = 6, 20, 32                      # two pixels
    dl = dr = np.full((H, W), d, np.int16)
    cl, cr = LR.lrc_confidence(dl, dr, None, INV, 24, 5, 2304)
    x = np.arange(W)[None, :].repeat(H, 0)
    assert np.array_equal(cl, np.where(x - 2 >= 0, 100, 0)) and np.array_equal(cr, np.where(x + 2 < W, 100, 0))
    base = np.full((H, W), 37, np.uint8)
    base[:, 5] = 11
    cl, cr = LR.lrc_confidence(dl, dr, base, INV, 24, 5, 2304)
    assert np.array_equal(cl, np.where(x - 2 >= 0, base, 0))            # base at the pixel itself
    assert cr[0, 3] == 11 and cr[0, 5] == 37 and cr[0, W - 2] == 0       # ... and, from the right view, at the matching left pixel


def test_planted_occlusion_band_and_mismatches_of_exactly_T_and_T_plus_1():
    H, W, d, T = 4, 40, 32, 24
    dl, dr = np.full((H, W), d, np.int16), np.full((H, W), d, np.int16)
    dr[:, 10:14] = INV                      # an occlusion band in the right view
    dr[1, 20] = d + T                       # differs by exactly T: kept
    dr[2, 20] = d + T + 1                   # by T + 1: cut
    dr[3, 20] = d - T - 1
    cl, cr = LR.lrc_confidence(dl, dr, None, INV, T, 0, 2304)
    want = np.full((H, W), 100, np.uint8)
    want[:, :2] = 0                         # the match leaves the image
    want[:, 12:16] = 0                      # left pixels whose match falls into the band
    want[2, 22] = want[3, 22] = 0           # the left pixels that look at column 20
    assert np.array_equal(cl, want) and cl[1, 22] == 100
    assert (cr[:, 10:14] == 0).all() and cr[0, 20] == 100 and cr[1, 20] == 100 and cr[2, 20] == 0 and cr[3, 20] == 0


def test_disparities_pointing_outside_the_image_on_both_sides():
    inv = -160                               # (minDisparity = -9: negative disparities are valid)
    dl = i16([[-48, -48, 0, 48, 48, -160]])  # -3, -3, 0, 3, 3 pixels, one invalid
    dr = np.full((1, 6), 0, np.int16)
    cl, cr = LR.lrc_confidence(dl, dr, None, inv, 32767, 0, 2304)
    # left x - d: 0 + 3 = 3, 1 + 3 = 4, 2, 3 - 3 = 0, 4 - 3 = 1: all inside;  the invalid pixel gives 0
    assert cl.tolist() == [[100, 100, 100, 100, 100, 0]]
    dl = i16([[48, -48, 0, -48, 48, 48]])
    cl, _ = LR.lrc_confidence(dl, dr, None, inv, 32767, 0, 2304)
    # 0 - 3 < 0: out;  1 + 3 = 4;  2;  3 + 3 = 6 >= W: out;  4 - 3 = 1;  5 - 3 = 2
    assert cl.tolist() == [[0, 100, 100, 0, 100, 100]]
    dr = i16([[-16, 0, 0, 0, 0, 16]])        # right x + d: 0 - 1 < 0: out;  5 + 1 >= W: out
    _, cr = LR.lrc_confidence(np.zeros((1, 6), np.int16), dr, None, inv, 32767, 0, 2304)
    assert cr.tolist() == [[0, 100, 100, 100, 100, 0]]


@pytest.mark.parametrize("d,shift", [(7, 0), (8, 1), (-8, 0), (-9, -1), (23, 1), (24, 2), (-24, -1), (-25, -2)])
def test_the_match_column_rounds_to_floor_of_d_plus_8_over_16(d, shift):
    inv, W, x = -160, 9, 4
    dl = np.full((1, W), inv, np.int16)
    dl[0, x] = d
    for k in range(-3, 4):                  # the right map valid at ONE column: the confidence says which one was looked at
        dr = np.full((1, W), inv, np.int16)
        dr[0, x - k] = d
        cl, _ = LR.lrc_confidence(dl, dr, None, inv, 0, 0, 2304)
        assert cl[0, x] == (100 if k == shift else 0), (d, k)
        cr_dl = np.full((1, W), inv, np.int16)   # and from the right view: x + shift
        cr_dl[0, x + k] = d
        _, cr = LR.lrc_confidence(cr_dl, dl, None, inv, 0, 0, 2304)
        assert cr[0, x] == (100 if k == shift else 0), (d, k)


def test_the_int64_extremes_stay_inside_int64():
    """maps alternating -32768 / 32767 at r = 16 (lrc_ref bounds every product with Python integers): with V = 1 the variance
    dwarfs V, with V = 2^30 it is about (32767.5)^2 = 2^30 - 32768, so the quotient is 99 or 100"""
    s = LR.extreme_pair(40, 70)
    assert (LR.smoothness(s["dl"], INV, 16, 1) == 0).all()
    F = LR.smoothness(s["dl"], INV, 16, 1 << 30)
    assert set(np.unique(F)) <= {0, 1} and (F == 1).any()
    one = np.full((40, 70), 32767, np.int16)                  # the largest s1^2 and n * s2, num = 0
    assert (LR.smoothness(one, INV, 16, 1) == 100).all()
    cl, cr = LR.lrc_confidence(s["dl"], s["dr"], s["base"], INV, 32767, 16, 1 << 30)
    assert cl.max() <= 1 and cr.max() <= 1


def test_left_and_right_confidence_mirror_each_other():
    """Mirror the pair by hand -- the right view flipped becomes a left view, with the same disparities -- and the left
    confidence of the mirrored pair is the flipped right confidence of the original (no base: it lives in one view)"""
    for seed, (H, W, r) in enumerate([(9, 40, 2), (33, 70, 5)]):
        s = LR.random_pair(H, W, 40 + seed)
        cl, cr = LR.lrc_confidence(s["dl"], s["dr"], None, INV, 24, r, 2304)
        ml, mr = LR.lrc_confidence(s["dr"][:, ::-1].copy(), s["dl"][:, ::-1].copy(), None, INV, 24, r, 2304)
        assert np.array_equal(ml[:, ::-1], cr) and np.array_equal(mr[:, ::-1], cl)
        assert (cl != 0).mean() > 0.25 and (cr != 0).mean() > 0.25


def test_the_generated_inputs_are_not_degenerate():
    """A condition on the INPUTS of the device tests, not a tolerance: every case of at least 64 x 64 pixels that uses T = 24 and
    V = 2304 has at least a quarter of its left confidences (with base, as generated) non-zero and at least 50 distinct values"""
    n = 0
    for i, (H, W, r, T, V, inv, levels) in enumerate(LR.SHAPE_CASES):
        if H * W >= 64 * 64 and T == 24 and V == 2304:
            cl, cr = LR.case_want(i)
            assert (cl != 0).mean() >= 0.25 and len(np.unique(cl)) >= 50, (H, W, (cl != 0).mean(), len(np.unique(cl)))
            assert (cr != 0).mean() >= 0.25 and len(np.unique(cr)) >= 50, (H, W)
            n += 1
    assert n >= 5
    shapes = [c[:2] for c in LR.SHAPE_CASES]
    for want in [(1, 1), (1, 7), (7, 1), (5, 63), (64, 64), (65, 129), (33, 200), (97, 260), (130, 67), (200, 33)]:
        assert want in shapes
    s = LR.case_input(2)                    # 7 x 1: its disparities do leave the image
    assert (LR.case_want(2)[0][s["dl"] >= INV + 16 + 8] == 0).all() and (s["dl"] >= INV + 16 + 8).any()


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_lrc.h")).read()
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", extra, flags=re.S))))
    assert declared == sorted(_lib.LRC_EXPORTS) == NEW
    assert '#include "sgm_hip_lrc.h"' in txt and all(hasattr(_lib.load(), n) for n in declared)
    for other in (_lib.EXPORTS, _lib.CONFIDENCE_EXPORTS, _lib.RIGHT_EXPORTS, _lib.WLS_EXPORTS, _lib.WLS_BATCH_EXPORTS):
        assert not set(_lib.LRC_EXPORTS) & set(other)
    assert sorted(_lib.WLS_BATCH_EXPORTS) == ["sgm_wls_filter_batch", "sgm_wls_filter_batch_device"]
    assert _lib.load().sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_lrc.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("lrc_confidence_host", "lrc_confidence_device", "lrc_confidence_batch_device"))
    assert callable(cv.lrcConfidence) and callable(cv.DisparityWLSFilter.getConfidenceMap)
    # what the documents must say: our own definition, not cv2's; ROI unbuilt
    for doc in (extra, cv.lrcConfidence.__doc__, cv.DisparityWLSFilter.__doc__):
        assert "NOT cv2" in doc.replace("\n", " ") and "ROI" in doc
    for stale in (open(os.path.join(ROOT, "include", "sgm_hip_wls.h")).read(), cv.DisparityWLSFilter.__doc__,
                  open(os.path.join(ROOT, "README.md")).read()):
        assert not re.search(r"depthDiscontinuityRadius\s+are\s+not\s+built", stale)


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU; so is N <= 0"""
    L = _lib.load()
    one = (np.ctypeslib.ctypes.c_void_p * 1)(8)
    for fn in (L.sgm_lrc_confidence, L.sgm_lrc_confidence_device):
        assert fn(None, 8, 16, None, 4, 4, -16, 24, 5, 2304, 24, None) == -1          # SGM_ERR_INVALID_ARG
        assert b"sgm_lrc_confidence" in L.sgm_last_error()
    assert L.sgm_lrc_confidence_batch_device(None, 1, one, one, None, 4, 4, -16, 24, 5, 2304, one, None) == -1
    assert L.sgm_lrc_confidence_batch_device(None, 0, one, one, None, 4, 4, -16, 24, 5, 2304, one, None) == -1
    assert b"N=0" in L.sgm_last_error()


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_setters_defaults_and_the_confidence_map_before_a_call(no_engine):
    f = cv.createDisparityWLSFilter()
    assert (f.getLRCthresh(), f.getDepthDiscontinuityRadius(), f.getDiscontinuityVariance()) == (24, 5, 2304)
    for bs, want in ((3, 2), (7, 4), (11, 6), (1, 1), (41, 16)):            # ceil(0.5 * blockSize), capped to 16
        assert cv.createDisparityWLSFilter(cv.StereoSGBM_create(blockSize=bs)).getDepthDiscontinuityRadius() == want
    with pytest.raises(cv.error, match="getConfidenceMap"):
        f.getConfidenceMap()
    for setter, bad, good in ((f.setLRCthresh, (-1, 32768, 2.5, "24", True, None), (0, 32767, np.int32(7))),
                              (f.setDepthDiscontinuityRadius, (-1, 17, 1.0, None), (0, 16, 3)),
                              (f.setDiscontinuityVariance, (0, -5, (1 << 30) + 1, 1e3), (1, 1 << 30, 64))):
        for v in bad:
            with pytest.raises(cv.error, match="not an integer in"):
                setter(v)
        for v in good:
            setter(v)
    assert (f.getLRCthresh(), f.getDepthDiscontinuityRadius(), f.getDiscontinuityVariance()) == (7, 3, 64)
    # a filter call WITHOUT a right map leaves no confidence map behind (it would need an engine to run: refused earlier)
    with pytest.raises(cv.error, match="CV_16SC1"):
        f.filter(np.zeros((4, 4), np.int32), np.zeros((4, 4), np.uint8))
    with pytest.raises(cv.error, match="getConfidenceMap"):
        f.getConfidenceMap()


def test_right_map_argument_errors_come_before_any_engine(no_engine):
    f = cv.createDisparityWLSFilter()
    d, g, c = np.zeros((6, 9), np.int16), np.zeros((6, 9), np.uint8), np.zeros((6, 9), np.uint8)
    with pytest.raises(cv.error, match="same size"):
        f.filter(d, g, c, disparity_map_right=d[:, :8])
    with pytest.raises(cv.error, match="same size"):
        f.filter(d, g, None, disparity_map_right=d[:5])
    with pytest.raises(cv.error, match="CV_16SC1"):
        f.filter(d, g, c, disparity_map_right=d.astype(np.int32))
    with pytest.raises(cv.error, match="CV_16SC1"):
        f.filter(d, g, c, disparity_map_right=d.astype(np.float32))
    import torch
    with pytest.raises(cv.error, match="CUDA"):
        f.filter(d, g, c, disparity_map_right=torch.from_numpy(d))
    # the batch form
    D, G = np.zeros((2, 6, 9), np.int16), np.zeros((2, 6, 9), np.uint8)
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(D, G, disparity_maps_right=D[:1])
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(D, G, disparity_maps_right=D[:, :, :8])
    with pytest.raises(cv.error, match="same size"):
        f.filterBatch(D, G, disparity_maps_right=[D[0], D[1, :5]])
    with pytest.raises(cv.error, match="CV_16SC1"):
        f.filterBatch(D, G, disparity_maps_right=D.astype(np.uint16))
    with pytest.raises(cv.error, match="CUDA"):
        f.filterBatch(D, G, disparity_maps_right=torch.from_numpy(D))
    # positional calls keep their meaning: the new keyword is the last parameter of both
    import inspect
    assert list(inspect.signature(f.filter).parameters)[-1] == "disparity_map_right"
    assert list(inspect.signature(f.filterBatch).parameters)[-1] == "disparity_maps_right"
    assert list(inspect.signature(f.filter).parameters)[:5] == ["disparity_map_left", "left_view", "confidence", "invalid", "return_float"]


def test_lrc_confidence_argument_errors_come_before_any_engine(no_engine):
    d, b = np.zeros((6, 9), np.int16), np.zeros((6, 9), np.uint8)
    with pytest.raises(cv.error, match="same size"):
        cv.lrcConfidence(d, d[:, :8])
    with pytest.raises(cv.error, match="same size"):
        cv.lrcConfidence(d, d, b[:5])
    with pytest.raises(cv.error, match="CV_16SC1"):
        cv.lrcConfidence(d, d.astype(np.int32))
    with pytest.raises(cv.error, match="CV_8UC1"):
        cv.lrcConfidence(d, d, b.astype(np.int16))
    with pytest.raises(cv.error, match=r"\(H, W\)"):
        cv.lrcConfidence(d[None], d[None])
    with pytest.raises(cv.error, match="empty"):
        cv.lrcConfidence(d[:0], d[:0])
    for kw in (dict(thresh=-1), dict(thresh=32768), dict(radius=17), dict(radius=-1), dict(var_max=0), dict(var_max=(1 << 30) + 1),
               dict(invalid=40000), dict(invalid=-32769), dict(radius=2.0)):
        with pytest.raises(cv.error, match="not an integer in"):
            cv.lrcConfidence(d, d, **kw)
    import torch
    with pytest.raises(cv.error, match="CUDA"):
        cv.lrcConfidence(torch.from_numpy(d), d)


def test_compute_filtered_refuses_an_unknown_confidence_before_any_engine(no_engine):
    m = cv.StereoSGBM_create(numDisparities=16)
    l = np.zeros((6, 40), np.uint8)
    for bad in ("nonsense", "LRC", "", None, 1):
        with pytest.raises(cv.error, match="'margin', 'lrc', 'both'"):
            m.computeFiltered(l, l, confidence=bad)
        with pytest.raises(cv.error, match="'margin', 'lrc', 'both'"):
            m.computeFilteredBatch(l[None], l[None], confidence=bad)
    import inspect
    for fn in (m.computeFiltered, m.computeFilteredBatch):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "confidence" and p["confidence"].default == "margin"
