"""The descriptor builder of Context.set_frames_device (superviseddescent_amd/_lib.py, frame_descriptors) on fake tensor objects:
pure host code, no device and no torch."""
import pytest

from superviseddescent_amd import _lib, frame_descriptors


class FakeTensor:
    """what the builder reads of a tensor: data_ptr(), shape, stride() (in elements) and dtype"""

    def __init__(self, ptr, shape, stride=None, dtype="torch.uint8"):
        self._ptr, self.shape, self.dtype = ptr, tuple(shape), dtype
        if stride is None:
            stride, acc = [], 1
            for n in reversed(self.shape):
                stride.insert(0, acc)
                acc *= n
        self._stride = tuple(stride)

    def data_ptr(self):
        return self._ptr

    def stride(self):
        return self._stride


def test_format_inference_from_the_shape():
    d = frame_descriptors([FakeTensor(1000, (40, 30)), FakeTensor(2000, (40, 30, 3)), FakeTensor(3000, (7, 5, 4))])
    assert d == [(1000, 30, 40, 30, _lib.SDM_FRAME_GRAY), (2000, 30, 40, 90, _lib.SDM_FRAME_BGR), (3000, 5, 7, 20, _lib.SDM_FRAME_BGRA)]
    # names, one for all or one per frame; None = the default of the shape
    assert frame_descriptors([FakeTensor(1, (4, 6, 3))], "rgb")[0][4] == _lib.SDM_FRAME_RGB
    d = frame_descriptors([FakeTensor(1, (4, 6, 3)), FakeTensor(2, (4, 6, 4)), FakeTensor(3, (4, 6))], ["RGB", "rgba", None])
    assert [f[4] for f in d] == [_lib.SDM_FRAME_RGB, _lib.SDM_FRAME_RGBA, _lib.SDM_FRAME_GRAY]
    assert frame_descriptors([FakeTensor(1, (4, 6))], "nv12")[0][4] == _lib.SDM_FRAME_NV12
    assert [_lib.SDM_FRAME_GRAY, _lib.SDM_FRAME_BGR, _lib.SDM_FRAME_RGB, _lib.SDM_FRAME_BGRA, _lib.SDM_FRAME_RGBA, _lib.SDM_FRAME_NV12] == list(range(6))


def test_views_keep_their_row_stride():
    # big[5:45, 8:40] of a 50 x 64 x 3 frame at 4096: pointer moved by the view, row stride that of the big frame
    roi = FakeTensor(4096 + 5 * 192 + 8 * 3, (40, 32, 3), (192, 3, 1))
    assert frame_descriptors([roi]) == [(4096 + 984, 32, 40, 192, _lib.SDM_FRAME_BGR)]
    gray = FakeTensor(77, (10, 9), (133, 1))
    assert frame_descriptors([gray]) == [(77, 9, 10, 133, _lib.SDM_FRAME_GRAY)]
    # dimensions of size 1 carry strides that are never used: accepted, and a one-row frame gets the dense stride
    assert frame_descriptors([FakeTensor(5, (1, 9), (0, 1))]) == [(5, 9, 1, 9, _lib.SDM_FRAME_GRAY)]
    assert frame_descriptors([FakeTensor(5, (3, 1, 3), (64, 999, 1))]) == [(5, 1, 3, 64, _lib.SDM_FRAME_BGR)]


def test_stacked_tensor_is_split_along_its_first_dimension():
    st = FakeTensor(10000, (3, 20, 16, 4))
    assert frame_descriptors(st, "rgba") == [(10000 + i * 20 * 16 * 4, 16, 20, 64, _lib.SDM_FRAME_RGBA) for i in range(3)]
    # a strided stack: every other frame of a pitched gray buffer
    st = FakeTensor(512, (2, 20, 16), (2 * 20 * 32, 32, 1))
    assert frame_descriptors(st) == [(512, 16, 20, 32, 0), (512 + 1280, 16, 20, 32, 0)]
    with pytest.raises(ValueError):
        frame_descriptors(FakeTensor(1, (20, 16)))                       # a single frame is passed in a list


def test_tuples_pass_through_unchanged():
    t = (0x7f0000001003, 1920, 1080, 2048, _lib.SDM_FRAME_NV12)
    assert frame_descriptors([t]) == [t]
    assert frame_descriptors([(123, 64, 48, 256, "nv12"), FakeTensor(9, (4, 4))], "gray") == [(123, 64, 48, 256, 5), (9, 4, 4, 4, 0)]
    # what the library refuses is the library's to refuse: the builder does not second-guess a ready descriptor
    assert frame_descriptors([(0, -1, 0, 1, 99)]) == [(0, -1, 0, 1, 99)]
    with pytest.raises(ValueError):
        frame_descriptors([(1, 2, 3, 4)])


def test_refusals():
    with pytest.raises(ValueError, match="stride"):
        frame_descriptors([FakeTensor(1, (8, 8), (16, 2))])                  # stride(-1) != 1: every other column
    with pytest.raises(ValueError, match="stride"):
        frame_descriptors([FakeTensor(1, (8, 8, 3), (64, 4, 1))])            # pixel stride 4 on 3 channels (a bgr view of bgra)
    with pytest.raises(ValueError, match="stride"):
        frame_descriptors([FakeTensor(1, (8, 8, 3), (24, 3, 2))])
    with pytest.raises(ValueError, match="stride"):
        frame_descriptors([FakeTensor(1, (8, 8, 3), (8, 1, 64))])            # planar data permuted to H x W x C
    with pytest.raises(ValueError, match="row stride"):
        frame_descriptors([FakeTensor(1, (8, 8, 3), (12, 3, 1))])            # overlapping rows
    for dtype in ("torch.int8", "torch.float32", "torch.uint16", "int32"):
        with pytest.raises(ValueError, match="uint8"):
            frame_descriptors([FakeTensor(1, (8, 8), dtype=dtype)])
    for shape in ((8, 8, 1), (8, 8, 2), (8, 8, 5), (8,), (2, 8, 8, 3, 1)):
        with pytest.raises(ValueError):
            frame_descriptors([FakeTensor(1, shape)])
    with pytest.raises(ValueError):
        frame_descriptors([FakeTensor(1, (8, 8, 3))], "gray")                # a format of another channel count
    with pytest.raises(ValueError):
        frame_descriptors([FakeTensor(1, (8, 8))], "bgr")
    with pytest.raises(ValueError):
        frame_descriptors([FakeTensor(1, (8, 8, 3))], "yuv")
    with pytest.raises(ValueError):
        frame_descriptors([FakeTensor(1, (8, 8, 3))], ["bgr", "bgr"])
    with pytest.raises(ValueError):
        frame_descriptors([])


def test_the_binding_declares_the_struct_of_the_header():
    import ctypes
    assert [n for n, _ in _lib.SdmFrame._fields_] == ["data", "width", "height", "stride_bytes", "format"]
    assert ctypes.sizeof(_lib.SdmFrame) == 24
    assert {"sdm_set_frames_device", "sdm_debug_download_image"} <= set(_lib.EXPORTED)
