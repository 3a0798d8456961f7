"""The YUV colour description without a device (include/sdm.h, "YUV colour description and 10-bit surfaces"): the shared device headers'
tables, decode, encode and P010 taps compiled for the host (tests/cpp/yuv_host.cpp, address and undefined-behaviour sanitizers) --
every table against the real value computed in double from Kr and Kb, value 5 against the functions it always was, the Python
restatement tests/yuv_ref.py bit for bit against the program, and the four P010 fetches on planes that live in heap blocks of exactly
the bytes the frame owns --, and the format names of the Python layer."""
import os
import struct

import numpy as np
import pytest

import cpp_build as B
import warp_ref as WR
import yuv_cases as C
import yuv_ref as Y
from superviseddescent_amd import _lib


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return B.host_program("yuv_host", tmp_path_factory.mktemp("yuv_host"))


def test_decode_8_bits_whole_cube(exe):
    """six tables x 256^3: every result within 0.501 of the clamped real value; value 5 the bits of align_nv12_to_bgr"""
    out = B.run(exe, ["decode8"], timeout=600, sanitized=True).stdout
    assert out.count("worst error") == 6 and "value 5 against align_nv12_to_bgr: 0 triples differ" in out


def test_decode_10_bits(exe):
    out = B.run(exe, ["decode10"], timeout=600, sanitized=True).stdout
    assert out.count("worst error") == 6


def test_encode_whole_cube_and_round_trip(exe):
    out = B.run(exe, ["encode"], timeout=600, sanitized=True).stdout
    assert out.count("round trip within") == 6 and "paste_nv12_chroma: 0 triples differ" in out


def test_constants_are_the_issues_check_values():
    """the REFERENCE's constants (tests/yuv_ref.py) against the published check values; the library's own tables are held to the
    same numbers inside the host program (decode8, decode10, encode), and to the reference bit for bit in the test below"""
    k = Y.decode_constants("bt709", False, 8)
    assert [k[n] for n in ("CY", "CVR", "CUB", "CVG", "CUG")] == [1220945, 1879825, 2215014, 558796, 223607]
    k = Y.decode_constants("bt709", False, 10)
    assert [k[n] for n in ("CY", "CVR", "CUB", "CVG", "CUG")] == [305236, 469956, 553753, 139699, 55902]
    e = Y.encode_constants("bt709", True)
    assert [e[n] for n in ("YR", "YG", "YB", "UB", "UG", "UR", "VR", "VG", "VB")] == \
        [222927, 749942, 75707, 524288, 404150, 120138, 524288, 476214, 48074]


def test_python_restatement_equals_the_host_program(exe, tmp_path):
    """2^16 random triples per table row: the 12 derived decodes and value 5's, the 6 derived encodes and value 5's"""
    n = 1 << 16
    tr = np.random.default_rng(5).integers(0, 1024, (n, 3), dtype=np.uint16)
    tr[:8] = [[1023 * (k & 1), 1023 * (k >> 1 & 1), 1023 * (k >> 2)] for k in range(8)]
    src, dst = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", n) + tr.tobytes())
    B.run(exe, ["dump", src, dst], timeout=300, sanitized=True)
    got = np.fromfile(dst, np.uint8).reshape(20, n, 3)
    t8, t10 = (tr & 255).astype(np.int64), tr.astype(np.int64)
    row = 0
    for depth, t in ((8, t8), (10, t10)):
        for m, full in Y.DESCRIPTIONS:
            want = Y.decode_with(Y.decode_constants(m, full, depth))(t[:, 0], t[:, 1], t[:, 2])
            assert np.array_equal(got[row], want), (depth, m, full)
            row += 1
    assert np.array_equal(got[row], Y.decode(Y.Desc("nv12"))(t8[:, 0], t8[:, 1], t8[:, 2]))
    row += 1
    for m, full in Y.DESCRIPTIONS + [(None, None)]:
        luma, chroma = (Y.luma_of(Y.Desc("nv12")), Y.chroma_of(Y.Desc("nv12"))) if m is None else \
            (Y.luma_with(Y.encode_constants(m, full)), Y.chroma_with(Y.encode_constants(m, full)))
        u, v = chroma(t8)
        assert np.array_equal(got[row], np.stack([luma(t8), u, v], -1)), (m, full)
        row += 1
    assert row == 20


def test_names_and_values():
    f = _lib._frame_format
    assert f("nv12") == 5 and f("nv12:bt601") == 5 and f("p010") == 7
    assert f("nv12:bt709") == 0x105 and f("nv12:bt601:full") == 0x1005 and f("p010:bt2020") == 0x207 and f("P010:BT2020:Full") == 0x1207
    for name in C.NAMES8 + C.NAMES10 + ["nv12", "p010"]:
        assert f(name) == Y.Desc(name).value, name
    for bad in ("bgr:bt709", "gray:full", "rgb_planar:bt709", "nv12:full:bt709", "nv12:bt709:bt2020", "p010:bt470", "nv12:bt709:full:full", "p011"):
        with pytest.raises(ValueError, match="unknown frame format"):
            f(bad)
    header = open(os.path.join(B.ROOT, "include", "sdm.h")).read()
    for line in ("#define SDM_FRAME_P010 7", "#define SDM_FRAME_BASE(f)       ((f) & 0xff)", "#define SDM_FRAME_YUV_BT709     0x100",
                 "#define SDM_FRAME_YUV_BT2020    0x200", "#define SDM_FRAME_YUV_FULL      0x1000"):
        assert line in header, line
    # tuples pass through with their description; an H x W uint8 tensor can be the luma of a described NV12 frame
    assert _lib.frame_descriptors([(64, 1920, 1080, 2048, "nv12:bt709"), (64, 1920, 1080, 4096, "p010:bt2020")]) == \
        [(64, 1920, 1080, 2048, 0x105), (64, 1920, 1080, 4096, 0x207)]


TAPS = [(1, 1), (2, 2), (5, 4), (38, 34)]


@pytest.mark.parametrize("pad", [0, 6])
def test_p010_fetches_on_blocks_of_exactly_the_frames_bytes(exe, tmp_path, pad):
    """rigid, area, warp and area warp, colour and luma-only, bit for bit against the restatement; faces over every border"""
    names = [C.NAMES10[i % 6] for i in range(len(TAPS))] if pad else [C.NAMES10[5 - i] for i in range(len(TAPS))]
    buf, frames = C.place([(w, h, name, pad, True) for (w, h), name in zip(TAPS, names)], seed=31 + pad)
    cw, ch = 11, 7
    lab = ((np.arange(ch)[:, None] + np.arange(cw)[None, :]) % 3).astype(np.uint8)
    lab[lab == 2] = WR.NONE
    seen = 0
    for k, f in enumerate(frames):
        fr = C.host_frame(buf, f)
        yb, uvb = C.plane_bytes(f)
        w, h = f["w"], f["h"]
        forms = [(1.0, 0.0, -0.7, -0.6), (0.61 * w / cw, 0.35, 0.1 * w, 0.4 * h), (2.3 * w / cw, -0.8, 0.3 * w, 0.2 * h), (-3.1, 3.4, w - 0.3, h - 0.4)]
        for n, (a, b, tx, ty) in enumerate(forms):
            M = np.array([a, -b, tx, b, a, ty], np.float32)
            M2 = np.array([0.5 * a, 0.3, tx + 0.25, -0.3, 0.7 * a, ty - 0.5], np.float32)
            S = 2 + n % 2
            samples = np.array([[1 + n % 3, 1 + n % 2], [3, 2]])
            case = struct.pack("<4i", f["desc"].value, w, h, f["stride"])
            case += struct.pack("<i", yb) + buf[f["off"]:f["off"] + yb].tobytes()
            case += struct.pack("<i", uvb) + buf[f["uv_off"]:f["uv_off"] + uvb].tobytes()
            case += struct.pack("<2i", cw, ch) + M.tobytes() + struct.pack("<2i", S, 2)
            for m, s in zip((M, M2), samples):
                case += m.tobytes() + struct.pack("<2i", int(s[0]), int(s[1]))
            case += struct.pack("<i", cw * ch) + lab.tobytes()
            src, dst = os.path.join(str(tmp_path), "case.bin"), os.path.join(str(tmp_path), "out.bin")
            with open(src, "wb") as fh:
                fh.write(case)
            B.run(exe, ["taps", src, dst], timeout=120, sanitized=True)
            got = np.fromfile(dst, np.uint8).reshape(4, ch * cw * 4)
            mats = np.stack([M, M2])
            want = [Y.rigid(fr, M, cw, ch), Y.area(fr, M, cw, ch, S), Y.warp(fr, mats, lab), Y.warp_area(fr, mats, lab, samples)]
            for i, (_, bgr, y8) in enumerate(want):
                assert np.array_equal(got[i, :ch * cw * 3].reshape(ch, cw, 3), bgr), (k, n, i, "colour")
                assert np.array_equal(got[i, ch * cw * 3:].reshape(ch, cw), y8), (k, n, i, "luma")
                seen += int(bgr.any())
    assert seen > 8 * len(frames)
