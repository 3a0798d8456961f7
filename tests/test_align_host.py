"""No-GPU checks of the aligned crops' host side: the C-ABI declarations of sdm_align_* and their export, the C++ header
rcr/alignment.hpp, the default template, and the host restatement (tests/align_ref.py) on known answers."""
import ctypes
import os
import re

import numpy as np

import align_ref as A
import cpp_build as B
from superviseddescent_amd import _lib, alignment_template, ibug

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_entry_points_are_declared_exported_and_bound(built):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdm.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("sdm_align_set_source", "sdm_align_crops"):
        assert re.search(r"\b%s\s*\(" % n, txt) and n in _lib.EXPORTED and hasattr(L, n)
    consts = dict(re.findall(r"#define (SDM_ALIGN_\w+) (\d+)", txt))
    assert {k: int(v) for k, v in consts.items()} == {"SDM_ALIGN_DEGENERATE": 1, "SDM_ALIGN_PARTIAL": 2}
    assert (_lib.SDM_ALIGN_DEGENERATE, _lib.SDM_ALIGN_PARTIAL) == (A.DEGENERATE, A.PARTIAL)


def test_alignment_header_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "rcr/alignment.hpp"\n'
                   'int main() {\n'
                   '    cv::Mat mean(1, 4, CV_32FC1);\n'
                   '    for (int i = 0; i < 4; ++i) mean.at<float>(i) = i % 2 ? 0.25f : -0.25f;\n'
                   '    cv::Mat t = rcr::alignment_template(mean, {0, 1}, 112, 96);\n'
                   '    return t.rows == 2 ? 0 : 1;\n'
                   '}\n')
    B.gpu_driver("t", tmp_path, src=src, opt=(), link=False)


def test_alignment_header_refuses_source_types_it_cannot_hold(tmp_path, built):
    """a colour source is packed into C bytes per pixel and cut into CV_8UC1 / CV_8UC3 crops: any other type (another depth, or a
    channel count without a crop type) is refused before the library is called"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "rcr/alignment.hpp"\n'
                   '#include <cstdio>\n'
                   'int main() {\n'
                   '    cv::Mat tmpl(2, 2, CV_32FC1);\n'
                   '    std::vector<cv::Mat> wrong{cv::Mat(8, 8, CV_32FC1)};\n'
                   '    try { rcr::detail::align_current_rows(nullptr, 1, {0, 1}, tmpl, 4, 4, wrong); }\n'
                   '    catch (const std::runtime_error& e) { std::printf("%s\\n", e.what()); return 0; }\n'
                   '    return 1;\n'
                   '}\n')
    out = B.run(B.gpu_driver("t", tmp_path, src=src, opt=()), [], 60)
    assert "CV_8UC1 or CV_8UC3" in out.stdout, out.stdout + out.stderr


def test_default_template():
    mean = ibug.select_mean(ibug.RCR22_IDS)
    L = mean.size // 2
    idx = np.arange(L)
    for w, h, margin in ((112, 112, 0.2), (96, 128, 0.1)):
        t = alignment_template(mean, idx, w, h, margin).astype(np.float64)
        assert t.shape == (L, 2) and t.dtype == np.float64
        lo, hi = t.min(0), t.max(0)
        assert np.allclose((lo + hi) / 2, [(w - 1) / 2, (h - 1) / 2], atol=1e-4)
        assert abs((hi - lo).max() - (1 - 2 * margin) * min(w, h)) < 1e-3
        # a similarity of the mean: the same shape, scaled
        m = np.stack([mean[:L], mean[L:]], 1).astype(np.float64)
        M, deg = A.fit64(np.concatenate([t[:, 0], t[:, 1]])[None], idx, m)
        assert not deg[0] and max(abs(M[0, 0, 1]), abs(M[0, 1, 0])) < 1e-4 * abs(M[0, 0, 0])      # (float32 template)


def test_fit_recovers_a_known_similarity():
    rng = np.random.default_rng(1)
    q = rng.uniform(10, 100, (9, 2)).astype(np.float32)
    idx = np.arange(9)
    for scale, ang in ((0.3, -45.0), (1.0, 0.0), (2.2, 17.0), (3.0, 45.0)):
        S = A.similarity(scale, ang, 40.0, -12.5)
        p = A.apply(S, q)
        row = np.concatenate([p[:, 0], p[:, 1]])[None]
        M, deg = A.fit64(row, idx, q)
        assert not deg[0]
        assert np.abs(M[0] - S).max() / np.abs(S).max() < 1e-5, (scale, ang)
    # coincident or non-finite landmarks: degenerate
    row = np.zeros((2, 18), np.float32)
    row[1] = np.concatenate([p[:, 0], p[:, 1]])
    row[1, 3] = np.nan
    M, deg = A.fit64(row, idx, q)
    assert deg.all() and np.isnan(M).all()


def test_identity_maps_to_a_byte_copy():
    rng = np.random.default_rng(2)
    for shape in ((37, 53), (20, 31, 3), (16, 9, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        crop = A.warp(img, np.array([[1, 0, 0], [0, 1, 0]], np.float32), shape[1], shape[0])
        assert np.array_equal(crop, img)
        assert not A.partial(np.array([[1, 0, 0], [0, 1, 0]], np.float32), shape[1], shape[0], shape[1], shape[0])
    # a whole-pixel shift moves the bytes and fills the rest with 0; half a pixel averages two neighbours (rounded)
    img = rng.integers(0, 256, (10, 12), dtype=np.uint8)
    crop = A.warp(img, np.array([[1, 0, 3], [0, 1, -2]], np.float32), 12, 10)
    assert np.array_equal(crop[2:, :9], img[:8, 3:]) and not crop[:2].any() and not crop[:, 9:].any()
    assert A.partial(np.array([[1, 0, 3], [0, 1, -2]], np.float32), 12, 10, 12, 10)
    half = A.warp(img, np.array([[1, 0, 0.5], [0, 1, 0]], np.float32), 11, 10)
    assert np.array_equal(half, ((img[:, :11].astype(int) * 512 + img[:, 1:].astype(int) * 512 + 512) >> 10).astype(np.uint8))
    # NaN or far-away positions give 0
    assert not A.warp(img, np.full((2, 3), np.nan, np.float32), 5, 5).any()
    assert not A.warp(img, np.array([[1, 0, 2.0 ** 21], [0, 1, 0]], np.float32), 5, 5).any()
