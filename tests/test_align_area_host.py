"""sdm_align_crops_tensor_filtered without a device: the S rule, the offset tables, what area sampling does to 1-pixel stripes and how
close it comes to the box integral of the bilinear surface, and the kernel's per-pixel code compiled for the host
(tests/cpp/align_area_host.cpp, address and undefined-behaviour sanitizers, planes of exactly the frames' bytes) against the numpy
restatement (tests/align_area_ref.py) on the device tests' frame sets."""
import ctypes
import struct

import numpy as np
import pytest

import align_area_cases as C
import align_area_ref as R
import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
from superviseddescent_amd import _lib, align_filter

f32 = np.float32


def test_s_rule():
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    for s2, want in ((1.0, 1), (up(1.0), 2), (4.0, 2), (up(4.0), 3), (255.9, 16), (256.0, 16), (300.0, 16), (np.inf, 1), (np.nan, 1),
                     (0.25, 1), (9.0, 3), (up(9.0), 4), (225.0, 15), (up(225.0), 16)):
        assert R.samples_of_s2(s2) == want, s2
    # the cap
    assert R.samples_of_s2(300.0, max_samples=4) == 4 and R.samples_of_s2(9.0, max_samples=2) == 2 and R.samples_of_s2(3.9, max_samples=1) == 1
    assert R.samples_of_s2(3.9, max_samples=2) == 2
    # the gate: s2 < min_scale^2 in float32 keeps S = 1; s2 == min_scale^2 does not
    assert R.samples_of_s2(3.9, min_scale=2.0) == 1 and R.samples_of_s2(4.0, min_scale=2.0) == 2 and R.samples_of_s2(up(4.0), min_scale=2.0) == 3
    assert R.samples_of_s2(6.2, min_scale=2.5) == 1 and R.samples_of_s2(6.25, min_scale=2.5) == 3
    assert R.samples_of_s2(200.0, min_scale=1e30) == 1                    # (min_scale^2 overflows to inf)
    # mode BILINEAR and a DEGENERATE row
    assert R.samples_of_s2(50.0, mode=R.BILINEAR) == 1 and R.samples_of_s2(50.0, degenerate=True) == 1
    # from a matrix: s2 = M00 M00 + M10 M10, each operation rounded
    M = A.similarity(2.6, 31.0, 5, 7).astype(f32)
    assert R.s2_of(M) == f32(f32(M[0, 0] * M[0, 0]) + f32(M[1, 0] * M[1, 0])) and R.samples(M) == 3
    assert R.samples(np.full((2, 3), np.nan, f32), degenerate=True) == 1


def test_offset_tables():
    for S in range(1, 17):
        o = R.offsets(S)
        assert o.dtype == np.float32 and o.shape == (S,)
        mirrored = -o[::-1]
        nz = o != 0                              # (an odd S has +0 in the middle, whose negation differs in the sign bit alone)
        assert np.array_equal(o[nz].view(np.uint32), mirrored[nz].view(np.uint32)) and np.all(o[~nz].view(np.uint32) == 0)
        assert (~nz).sum() == S % 2 and float(o.astype(np.float64).sum()) == 0.0
        assert np.all(np.diff(o) > 0) and abs(float(o[0])) < 0.5
        exact = (2 * np.arange(S) + 1 - S) / (2.0 * S)
        assert np.array_equal(o, exact.astype(f32))                       # the float64 quotient rounded once is the float32 quotient
    assert np.array_equal(R.offsets(1).view(np.uint32), np.zeros(1, np.uint32))


def test_filter_from_named_options():
    f = align_filter()
    assert (f.mode, f.max_samples, f.min_scale) == (_lib.SDM_ALIGN_FILTER_AREA, 16, 1.0)
    f = align_filter("bilinear", 4, 2.5)
    assert (f.mode, f.max_samples, f.min_scale) == (_lib.SDM_ALIGN_FILTER_BILINEAR, 4, 2.5)
    assert ctypes.sizeof(_lib.SdmAlignFilter) == 12 and ctypes.sizeof(_lib.SdmAlignTensor) == 44
    assert "sdm_align_crops_tensor_filtered" in _lib.EXPORTED
    for kw in (dict(mode="box"), dict(mode=None), dict(max_samples=0), dict(max_samples=17), dict(max_samples=2.5), dict(min_scale=0.5),
               dict(min_scale=np.inf), dict(min_scale=np.nan)):
        with pytest.raises(ValueError):
            align_filter(**kw)


def test_s1_is_the_bilinear_restatement():
    buf, frames = K.place(K.RAGGED, 11)
    for f, S in zip(frames, K.similarities(frames, range(len(frames)), 7, 7, 3)):
        M = S.astype(f32)
        frame = K.host_frame(buf, f)
        kind, bgr = T.warped(frame, M, 7, 7)
        k2, b2, _ = R.warped(frame, M, 7, 7, 1)
        assert kind == k2 and np.array_equal(bgr, b2)


@pytest.mark.parametrize("scale", [4, 8])
def test_stripes(scale):
    frame, x, tmpl, w, h, M_want = C.stripes(scale)
    M, degenerate = A.fit64(x, C.LM, tmpl)
    assert not degenerate[0] and np.array_equal(M[0], M_want)            # the fit is exactly [[s, 0, tx], [0, s, ty]]
    M = M[0].astype(f32)
    S = R.samples(M)
    assert S == scale
    _, area, _ = R.warped(T.Frame(T.GRAY, frame), M, w, h, S)
    _, plain = T.warped(T.Frame(T.GRAY, frame), M, w, h)
    assert np.all(area == 128)                                            # every footprint lies inside the frame: all pixels are interior
    assert set(np.unique(plain)) <= {0, 255}                              # (an even scale steps over one parity of columns)


def ideal_box(img, M, width, height, n=32):
    """float64 box integral of the bilinear surface over every crop pixel's footprint, n x n midpoints; (values, footprint inside)"""
    M = np.asarray(M, np.float64)
    o = (np.arange(n) + 0.5) / n - 0.5
    fj = np.arange(width)[None, :, None, None] + o[None, None, None, :]
    fi = np.arange(height)[:, None, None, None] + o[None, None, :, None]
    sx = M[0, 0] * fj + M[0, 1] * fi + M[0, 2]
    sy = M[1, 0] * fj + M[1, 1] * fi + M[1, 2]
    H, W = img.shape
    inside = ((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).all((2, 3))
    x0 = np.clip(np.floor(sx).astype(int), 0, W - 2)
    y0 = np.clip(np.floor(sy).astype(int), 0, H - 2)
    ax, ay = np.clip(sx - x0, 0, 1), np.clip(sy - y0, 0, 1)
    g = img.astype(np.float64)
    v = (1 - ax) * (1 - ay) * g[y0, x0] + ax * (1 - ay) * g[y0, x0 + 1] + (1 - ax) * ay * g[y0 + 1, x0] + ax * ay * g[y0 + 1, x0 + 1]
    return v.mean((2, 3)), inside


def test_closer_to_the_ideal_than_bilinear():
    img = np.random.default_rng(5).integers(0, 256, (96, 96), dtype=np.uint8)
    frame = T.Frame(T.GRAY, img)
    w = h = 8
    for scale in (2.5, 4.3, 7.0):
        for angle in (0.0, 17.0, 45.0):
            S64 = A.similarity(scale, angle, 0, 0)
            S64[:, 2] = np.array([47.3, 48.1]) - S64[:, :2] @ np.array([(w - 1) / 2, (h - 1) / 2])
            M = S64.astype(f32)
            S = R.samples(M)
            assert S == int(np.ceil(scale))
            ideal, inside = ideal_box(img, M, w, h)
            assert inside.sum() >= 16
            _, area, _ = R.warped(frame, M, w, h, S)
            _, plain = T.warped(frame, M, w, h)
            e_area = np.abs(area[..., 0] - ideal)[inside].mean()
            e_plain = np.abs(plain[..., 0] - ideal)[inside].mean()
            print("scale %.1f angle %2.0f S %d: mean |error| against the box integral, area %.3f, bilinear %.3f (%d pixels)"
                  % (scale, angle, S, e_area, e_plain, inside.sum()))
            assert e_area < e_plain


def test_host_build_of_the_pixel_code_under_sanitizers(tmp_path):
    """the device functions, compiled for the host with their own main, on planes of exactly the frames' bytes.  The host program also
    runs every segment through the 64-bit offset path (WIDE) and compares: no frame set of the device tests has a plane beyond INT_MAX
    bytes, so this is where that path is covered."""
    exe = B.host_program("align_area_host", tmp_path)
    scale, bias = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], f32), np.array([-2.1179, -2.0357, -1.8044], f32)
    cases, blob, seen = [], [b""], set()
    for specs, seed in ((K.RAGGED, 11), (K.NV12, 12)):
        buf, frames = K.place(specs, seed)
        for (w, h) in K.CROPS:
            for f in frames:
                for v, (S64, filt, want) in enumerate(C.variants(f, w, h, seed + w)):
                    M = S64.astype(f32)
                    mode, max_samples, min_scale = filt
                    b0, b1 = K.plane_bytes(f)
                    blob.append(struct.pack("<7i", f["fmt"], f["w"], f["h"], f["stride"], f["stride"] if b1 else 0, w, h) + M.tobytes()
                                + scale.tobytes() + bias.tobytes() + struct.pack("<iif", mode, max_samples, min_scale)
                                + struct.pack("<i", b0) + buf[f["off"]:f["off"] + b0].tobytes()
                                + struct.pack("<i", b1) + (buf[f["uv_off"]:f["uv_off"] + b1].tobytes() if b1 else b""))
                    S = R.samples(M, False, mode, max_samples, min_scale)
                    assert S == want, (v, S, want)
                    cases.append((K.host_frame(buf, f), M, w, h, S))
                    seen.add((f["fmt"], S))
    assert seen >= {(fmt, S) for fmt in range(6) for S in (1, 2, 3, 4, 5, 16)}          # every format at every S
    blob[0] = struct.pack("<i", len(cases))
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 300, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at = 0
    for frame, M, w, h, S in cases:
        assert int(got[at:at + 4].view(np.int32)[0]) == S
        at += 4
        kind, bgr, y = R.warped(frame, M, w, h, S)
        n = w * h
        assert np.array_equal(got[at:at + 3 * n].reshape(h, w, 3), bgr), (frame.fmt, frame.w, frame.h, w, h, S)
        at += 3 * n
        for shift in (14, 15):
            want = T.finish(kind, bgr, y, "uint8", "nhwc", 1, "bgr", gray_shift=shift)[..., 0]
            assert np.array_equal(got[at:at + n].reshape(h, w), want), (frame.fmt, shift, S)
            at += n
        want = T.finish(kind, bgr, None, "float32", "nchw", 3, "rgb", scale, bias)
        assert np.array_equal(got[at:at + 12 * n].copy().view(np.uint32).reshape(3, h, w), want.view(np.uint32)), (frame.fmt, S)
        at += 12 * n
    assert at == got.size
