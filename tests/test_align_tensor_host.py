"""sdm_align_crops_tensor without a device: the restated NV12 conversion over all 256^3 inputs, the element formula against float64,
the Python argument handling on fake tensors, and the kernel's per-pixel code compiled for the host (tests/cpp/align_tensor_host.cpp,
address and undefined-behaviour sanitizers, planes of exactly the frames' bytes) against the numpy restatement on the device tests'
frame sets."""
import struct

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
from superviseddescent_amd import _lib, align_tensor_spec

f32 = np.float32


def test_nv12_conversion_all_inputs_clamp_and_int32():
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0
    for Y in range(256):
        bgr = T.nv12_to_bgr(Y, U, V)
        assert bgr.min() >= 0 and bgr.max() <= 255
        terms, sums = T.nv12_terms(Y, U, V)
        for t in terms:
            assert np.abs(t).max() < 2 ** 30                       # every term below 2^30 in magnitude
        for s in sums:
            assert -T.INT32 <= s.min() and s.max() < T.INT32       # every partial sum is an int32
            worst = max(worst, int(np.abs(s).max()))
    print("largest |sum| before the shift:", worst)
    # the clamp is needed on both sides: saturated chroma leaves [0, 255] before it
    y = np.int64(max(0, 235 - 16) * 1220542)
    assert (y + 2116026 * (255 - 128) + (1 << 19)) >> 20 > 255 and (np.int64(0) + 2116026 * (0 - 128) + (1 << 19)) >> 20 < 0


def test_nv12_neutral_chroma_is_gray():
    Y = np.arange(256)
    bgr = T.nv12_to_bgr(Y, 128, 128)
    want = (np.maximum(0, Y - 16) * 1220542 + (1 << 19)) >> 20
    assert want.max() > 255                                        # (Y above 235: super-white, clamped)
    for c in range(3):
        assert np.array_equal(bgr[..., c], np.clip(want, 0, 255))


def test_element_formula_against_float64():
    v = np.arange(256)
    pairs = [(f32(1 / 58.395), f32(-2.1179)), (f32(1 / 255.0), f32(0.0)), (f32(0.0078125), f32(-1.0))]
    undecided = 0
    for scale, bias in pairs:
        e32 = T.element(v, scale, bias, "float32")
        e16 = T.element(v, scale, bias, "float16")
        assert e32.dtype == np.float32 and e16.dtype == np.float16
        exact = v.astype(np.float64) * np.float64(scale) + np.float64(bias)      # exact: 8 x 24 bits, then a sum of two doubles
        once = exact.astype(np.float16)
        # float32's two roundings cannot interfere when the exact value and the float32 value lie strictly inside the interval that
        # rounds to `once`: between the midpoints to its float16 neighbours
        up = (once.astype(np.float64) + np.nextafter(once, np.float16(np.inf)).astype(np.float64)) / 2
        dn = (once.astype(np.float64) + np.nextafter(once, np.float16(-np.inf)).astype(np.float64)) / 2
        lo, hi = np.minimum(exact, e32.astype(np.float64)), np.maximum(exact, e32.astype(np.float64))
        safe = (lo > dn) & (hi < up)
        assert np.array_equal(e16[safe].view(np.uint16), once[safe].view(np.uint16))
        undecided += int((~safe).sum())
    print("element formula: %d of %d values on a float16 rounding boundary (not compared)" % (undecided, 256 * len(pairs)))
    # (float32 is within 2^-13 of a float16 spacing of the exact value: boundaries are rare, and the comparison above is not vacuous)
    assert undecided < 256 * len(pairs) // 4


class FakeOut:
    def __init__(self, shape, dtype="torch.float16", contiguous=True, cuda=True):
        self.shape, self.dtype, self._c, self.is_cuda = tuple(shape), dtype, contiguous, cuda

    def is_contiguous(self):
        return self._c


def test_spec_from_named_options():
    s = align_tensor_spec()
    assert (s.dtype, s.layout, s.channels, s.order, s.gray_shift) == (_lib.SDM_ALIGN_F16, _lib.SDM_ALIGN_NCHW, 3, _lib.SDM_ALIGN_ORDER_RGB, 14)
    assert list(s.scale) == [1.0] * 3 and list(s.bias) == [0.0] * 3
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    s = align_tensor_spec(mean=mean, std=std)
    assert [f32(v) for v in s.scale] == [f32(1 / d) for d in std]
    assert [f32(v) for v in s.bias] == [f32(-m / d) for m, d in zip(mean, std)]
    s = align_tensor_spec(mean=127.5, std=128)                                   # scalars go to all three channels
    assert list(s.scale) == [0.0078125] * 3 and [f32(v) for v in s.bias] == [f32(-127.5 / 128)] * 3
    s = align_tensor_spec(std=2.0)
    assert list(s.scale) == [0.5] * 3 and list(s.bias) == [0.0] * 3
    s = align_tensor_spec("uint8", "NHWC", 1, "BGR", scale=[1, 2, 3], bias=0.5, gray_shift=15)
    assert (s.dtype, s.layout, s.channels, s.order, s.gray_shift) == (_lib.SDM_ALIGN_U8, _lib.SDM_ALIGN_NHWC, 1, _lib.SDM_ALIGN_ORDER_BGR, 15)
    assert list(s.scale) == [1.0, 2.0, 3.0] and list(s.bias) == [0.5] * 3
    assert align_tensor_spec(np.float32).dtype == _lib.SDM_ALIGN_F32 and align_tensor_spec("torch.float32").dtype == _lib.SDM_ALIGN_F32
    import ctypes
    assert ctypes.sizeof(_lib.SdmAlignTensor) == 44
    assert {"sdm_align_set_source_frames", "sdm_align_crops_tensor"} <= set(_lib.EXPORTED)


def test_spec_refusals():
    for kw in (dict(mean=1.0, scale=1.0), dict(std=2.0, bias=0.0), dict(mean=1.0, std=2.0, scale=1.0, bias=1.0),
               dict(dtype="int8"), dict(dtype="float64"), dict(layout="chw"), dict(layout=1), dict(order="gbr"), dict(order=None),
               dict(channels=4), dict(channels=2), dict(gray_shift=13), dict(scale=[1, 2]), dict(bias=[1, 2, 3, 4]), dict(std=[1, 0, 1]),
               dict(mean=[1, 2])):
        with pytest.raises(ValueError):
            align_tensor_spec(**kw)


def test_out_tensor_is_checked():
    shape = _lib.align_tensor_shape(5, 16, 12, _lib.SDM_ALIGN_NCHW, 3)
    assert shape == (5, 3, 12, 16) and _lib.align_tensor_shape(5, 16, 12, _lib.SDM_ALIGN_NHWC, 1) == (5, 12, 16, 1)
    _lib.check_align_out(FakeOut(shape), shape, "float16")
    for bad in (FakeOut(shape, "torch.float32"), FakeOut((5, 12, 16, 3)), FakeOut(shape[1:]), FakeOut(shape, contiguous=False),
                FakeOut(shape, cuda=False)):
        with pytest.raises(ValueError):
            _lib.check_align_out(bad, shape, "float16")


def test_host_build_of_the_pixel_code_under_sanitizers(tmp_path):
    """the device functions, compiled for the host with their own main, on planes of exactly the frames' bytes"""
    exe = B.host_program("align_tensor_host", tmp_path)
    scale, bias = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], f32), np.array([-2.1179, -2.0357, -1.8044], f32)
    cases, blob = [], [b""]
    for specs, seed in ((K.RAGGED, 11), (K.NV12, 12)):
        buf, frames = K.place(specs, seed)
        for (w, h) in K.CROPS:
            sims = K.similarities(frames, range(len(frames)), w, h, seed + w)
            for f, S in zip(frames, sims):
                M = S.astype(f32)
                b0, b1 = K.plane_bytes(f)
                blob.append(struct.pack("<7i", f["fmt"], f["w"], f["h"], f["stride"], f["stride"] if b1 else 0, w, h) + M.tobytes()
                            + scale.tobytes() + bias.tobytes() + struct.pack("<i", b0) + buf[f["off"]:f["off"] + b0].tobytes()
                            + struct.pack("<i", b1) + (buf[f["uv_off"]:f["uv_off"] + b1].tobytes() if b1 else b""))
                cases.append((K.host_frame(buf, f), M, w, h))
    blob[0] = struct.pack("<i", len(cases))
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 120, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at = 0
    for frame, M, w, h in cases:
        kind, bgr = T.warped(frame, M, w, h)
        n = w * h
        assert np.array_equal(got[at:at + 3 * n].reshape(h, w, 3), bgr), (frame.fmt, frame.w, frame.h, w, h)
        at += 3 * n
        for shift in (14, 15):
            want = T.finish(kind, bgr, bgr[..., 0], "uint8", "nhwc", 1, "bgr", gray_shift=shift)[..., 0]
            assert np.array_equal(got[at:at + n].reshape(h, w), want), (frame.fmt, shift)
            at += n
        want = T.finish(kind, bgr, None, "float32", "nchw", 3, "rgb", scale, bias)
        assert np.array_equal(got[at:at + 12 * n].view(np.uint32).reshape(3, h, w), want.view(np.uint32)), frame.fmt
        at += 12 * n
    assert at == got.size
