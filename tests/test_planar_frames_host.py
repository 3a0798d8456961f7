"""Planar colour frames (include/sdm.h, "Planar colour frames") in the descriptor builder of every ``frames=`` call
(superviseddescent_amd/_lib.py, frame_planes / frame_descriptors) on fake tensor objects: pure host code, no device and no torch."""
import ctypes

import pytest

from superviseddescent_amd import _lib, frame_descriptors
from test_frames_host import FakeTensor


def frame_planes(*args, **kwargs):
    return _lib.frame_planes(*args, **kwargs)


BP, RP = 16, 17


def test_the_format_codes_and_names():
    assert (_lib.SDM_FRAME_BGR_PLANAR, _lib.SDM_FRAME_RGB_PLANAR) == (BP, RP)
    assert _lib.FRAME_FORMATS["bgr_planar"] == BP and _lib.FRAME_FORMATS["rgb_planar"] == RP
    assert 6 not in _lib.FRAME_FORMATS.values()
    assert "sdm_set_frames_device_planes" in _lib.EXPORTED
    header = open(_lib_header()).read()
    assert "#define SDM_FRAME_BGR_PLANAR 16" in header and "#define SDM_FRAME_RGB_PLANAR 17" in header
    assert "sdm_set_frames_device_planes(" in header


def _lib_header():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdm.h")


def test_a_named_tensor_is_one_planar_frame_with_the_default_plane_distance():
    t = FakeTensor(4096, (3, 40, 30))
    for name, code in (("bgr_planar", BP), ("RGB_PLANAR", RP), (RP, RP)):
        desc, planes = frame_planes([t], name)
        assert desc == [(4096, 30, 40, 30, code)] and planes == [None]
        assert frame_descriptors([t], name) == desc                       # 5-tuples, as ever
    # one bare 3 x H x W tensor with a planar name is one frame, not a stack of three gray ones
    assert frame_planes(t, "rgb_planar") == ([(4096, 30, 40, 30, RP)], [None])
    assert frame_planes(t, ["rgb_planar"]) == ([(4096, 30, 40, 30, RP)], [None])          # ... also with its name in a list of one
    assert _lib._one_planar_name("rgb_planar") == "rgb_planar" and _lib._one_planar_name([BP]) == BP
    assert _lib._one_planar_name("rgb") is None and _lib._one_planar_name(None) is None and _lib._one_planar_name(["bgr_planar"] * 2) is None
    with pytest.raises(ValueError):
        frame_planes(t, ["rgb_planar"] * 2)                                                # (a stack of three: one format per frame)
    # one name per frame: planar beside interleaved, gray and a tuple
    desc, planes = frame_planes([t, FakeTensor(1, (8, 6, 3)), FakeTensor(2, (8, 6)), (9, 64, 48, 256, "nv12")],
                                ["rgb_planar", "rgb", None, None])
    assert [d[4] for d in desc] == [RP, _lib.SDM_FRAME_RGB, _lib.SDM_FRAME_GRAY, _lib.SDM_FRAME_NV12] and planes == [None] * 4


def test_row_and_channel_strides_are_free():
    # a region x[:, 5:45, 8:40] of a 3 x 50 x 64 tensor at 1000: pointer moved by the view, strides those of the big tensor
    roi = FakeTensor(1000 + 5 * 64 + 8, (3, 40, 32), (50 * 64, 64, 1))
    assert frame_planes([roi], "bgr_planar") == ([(1328, 32, 40, 64, BP)], [1328 + 3200])
    # a padded channel stride (an odd one: the planes are misaligned against each other)
    pad = FakeTensor(512, (3, 9, 17), (9 * 20 + 3, 20, 1))
    assert frame_planes([pad], "rgb_planar") == ([(512, 17, 9, 20, RP)], [512 + 183])
    # a channel-reversed view x.flip(0) as a foreign library hands it out: negative channel stride, pointer at the last plane
    rev = FakeTensor(9000 + 2 * 600, (3, 20, 30), (-600, 30, 1))
    assert frame_planes([rev], "bgr_planar") == ([(10200, 30, 20, 30, BP)], [10200 - 600])
    # a channel-sliced buffer: planes 0, 1, 2 of a 4-plane block with its own pitch
    sl = FakeTensor(64, (3, 8, 8), (8 * 16, 16, 1))
    assert frame_planes([sl], "bgr_planar") == ([(64, 8, 8, 16, BP)], [None])         # 8 rows of 16: the default distance
    # dimensions of size 1 carry strides that are never used
    assert frame_planes([FakeTensor(5, (3, 1, 9), (40, 0, 1))], "bgr_planar") == ([(5, 9, 1, 9, BP)], [45])
    assert frame_planes([FakeTensor(5, (3, 4, 1), (4 * 7, 7, 999))], "bgr_planar") == ([(5, 1, 4, 7, BP)], [None])
    # a channel stride of 0 (an expanded gray plane) is the library's to refuse: the second plane lies on the first
    assert frame_planes([FakeTensor(5, (3, 4, 4), (0, 4, 1))], "bgr_planar")[1] == [5]


def test_refusals_of_a_named_tensor():
    with pytest.raises(ValueError, match=r"stride\(2\)"):
        frame_planes([FakeTensor(1, (3, 8, 8), (64, 16, 2))], "bgr_planar")            # every other column
    with pytest.raises(ValueError, match=r"stride\(2\)"):
        frame_planes([FakeTensor(1, (3, 8, 8), (1, 24, 3))], "rgb_planar")             # interleaved data permuted to 3 x H x W
    with pytest.raises(ValueError, match="row stride"):
        frame_planes([FakeTensor(1, (3, 8, 8), (64, 4, 1))], "bgr_planar")             # overlapping rows
    for shape in ((8, 8, 3), (4, 8, 8), (1, 8, 8), (8, 8), (1, 3, 8, 8)):
        with pytest.raises(ValueError):
            frame_planes([FakeTensor(1, shape)], "bgr_planar")
    with pytest.raises(ValueError, match="uint8"):
        frame_planes([FakeTensor(1, (3, 8, 8), dtype="torch.float32")], "rgb_planar")
    with pytest.raises(ValueError):
        frame_planes([FakeTensor(1, (3, 8, 8))], "planar")
    with pytest.raises(ValueError):
        frame_planes([FakeTensor(1, (3, 0, 8))], "bgr_planar")


def test_a_stacked_batch_splits_along_dimension_0():
    st = FakeTensor(10000, (4, 3, 20, 16))
    desc, planes = frame_planes(st, "rgb_planar")
    assert desc == [(10000 + i * 960, 16, 20, 16, RP) for i in range(4)] and planes == [None] * 4
    # every other frame of a pitched batch whose planes are padded
    st = FakeTensor(512, (2, 3, 20, 16), (2 * 3 * 700, 700, 32, 1))
    desc, planes = frame_planes(st, "bgr_planar")
    assert desc == [(512, 16, 20, 32, BP), (512 + 4200, 16, 20, 32, BP)] and planes == [512 + 700, 512 + 4200 + 700]
    # without the name a 4-dimensional stack is n x H x W x C, as ever: 3 x 20 x 16 frames of 16 channels are refused
    with pytest.raises(ValueError):
        frame_planes(st)


def test_tuples_take_their_second_plane_from_chroma():
    t = (0x7f0000001003, 1920, 1080, 2048, "rgb_planar")
    assert frame_planes([t]) == ([(0x7f0000001003, 1920, 1080, 2048, RP)], [None])
    assert frame_planes([t, (77, 4, 4, 4, BP)], chroma=[0x7f0000001003 - 4096, None]) == \
        ([(0x7f0000001003, 1920, 1080, 2048, RP), (77, 4, 4, 4, BP)], [0x7f0000001003 - 4096, None])
    # a uint8 tensor as the second plane; an NV12 tuple's UV plane travels in the same list
    uv = FakeTensor(555, (540, 1920))
    assert frame_planes([(100, 1920, 1080, 1920, "nv12"), t], chroma=[uv, FakeTensor(31, (1080, 1920))])[1] == [555, 31]
    # an entry given for a planar tensor replaces the one computed from its strides
    assert frame_planes([FakeTensor(8, (3, 4, 4))], "bgr_planar", chroma=[99])[1] == [99]
    with pytest.raises(ValueError, match="chroma"):
        frame_planes([t], chroma=[1, 2])
    # frame_descriptors keeps passing ready descriptors through
    assert frame_descriptors([t]) == [(0x7f0000001003, 1920, 1080, 2048, RP)]


def test_an_unnamed_tensor_behaves_as_before():
    # 3 x H x W without a planar name: H x W x C with H = 3 -- never planar
    with pytest.raises(ValueError):
        frame_descriptors([FakeTensor(1, (3, 8, 8))])                              # 8 channels
    assert frame_descriptors([FakeTensor(1, (3, 8, 4))]) == [(1, 8, 3, 32, _lib.SDM_FRAME_BGRA)]
    assert frame_planes([FakeTensor(1, (3, 8, 4))]) == ([(1, 8, 3, 32, _lib.SDM_FRAME_BGRA)], [None])
    with pytest.raises(ValueError, match="stride"):
        frame_descriptors([FakeTensor(1, (8, 8, 3), (8, 1, 64))])                  # planar data permuted to H x W x C
    with pytest.raises(ValueError):
        frame_descriptors([FakeTensor(1, (3, 8, 8))], "rgb")
    # a bare 3-dimensional tensor without a planar name is a stack of gray frames
    assert frame_descriptors(FakeTensor(0, (3, 8, 8))) == [(i * 64, 8, 8, 8, 0) for i in range(3)]


def test_planes_array():
    assert _lib.planes_array([None, None]) is None
    a = _lib.planes_array([None, 4096, 7])
    assert isinstance(a, ctypes.Array) and [a[0], a[1], a[2]] == [None, 4096, 7]
