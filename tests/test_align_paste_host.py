"""sdm_align_paste_tensor without a device: the kernel's per-pixel code and its prepare stage compiled for the host
(tests/cpp/align_paste_host.cpp, address and undefined-behaviour sanitizers, every frame, tensor and opacity map in a heap block of
exactly its bytes) against the numpy restatement (tests/paste_ref.py), bit for bit on every byte the frame owns; the restatement's own
blend identities; the Python argument handling."""
import itertools
import struct

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import paste_cases as C
import paste_ref as P
from superviseddescent_amd import _lib

f32 = np.float32
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))


def test_blend_identities():
    o, q = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal((255 * q + 0 * o + 127) // 255, q)                  # a = 255: the sampled colour
    for a in range(1, 255):
        new = (a * q + (255 - a) * o + 127) // 255
        assert new.min() >= 0 and new.max() <= 255
        assert np.array_equal(new[o == q], o[o == q])                         # a colour blended with itself stays
        assert (np.abs(new - o) <= np.abs(q - o)).all()


def test_decode_clamps_rounds_to_even_and_drops_nan():
    x = np.array([[-1.0], [0.5], [1.5], [2.5], [254.5], [255.5], [300.0], [np.nan], [np.inf], [-np.inf]], f32)
    assert P.decode(x, 1.0, 0.0)[:, 0].tolist() == [0, 0, 2, 2, 254, 255, 255, 0, 255, 0]
    assert P.decode(x.astype(np.float16), 2.0, 1.0)[:, 0].tolist() == [0, 2, 4, 6, 255, 255, 255, 0, 255, 0]
    assert P.decode(np.array([[7]], np.uint8), 3.0, 9.0)[0, 0] == 7             # scale and bias do not touch bytes


def test_inverse_and_flags():
    W, bad = P.inverse([[2, 0, 3], [0, 4, 5]])
    assert not bad and W.tolist() == [0.5, 0, -1.5, 0, 0.25, -1.25]
    assert P.inverse([[1, 2, 3], [2, 4, 1]])[1] and P.inverse([[1, 0, np.nan], [0, 1, 0]])[1]
    assert P.flags_at([[1, 0, np.nan], [0, 1, 0]], 4, 4, 8, 8) == A.DEGENERATE
    assert P.flags_at([[1, 2, 3], [2, 4, 1]], 4, 4, 8, 8) == A.DEGENERATE | A.PARTIAL
    assert P.flags_at([[1, 0, 1], [0, 1, 1]], 4, 4, 8, 8) == 0 and P.flags_at([[1, 0, 5], [0, 1, 1]], 4, 4, 8, 8) == A.PARTIAL


def test_symbols_struct_and_feather_mask():
    import ctypes
    from superviseddescent_amd import feather_mask
    assert {"sdm_align_paste_tensor", "sdm_align_paste_tensor_at"} <= set(_lib.EXPORTED)
    assert ctypes.sizeof(_lib.SdmAlignPaste) == 16
    m = feather_mask(8, 2)
    assert m.dtype == np.uint8 and m.shape == (8, 8) and m[3, 3] == 255 and m[0, 4] < m[1, 4] < m[2, 4] == 255 and m[0, 0] <= m[0, 4]
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1, ::-1])
    assert feather_mask((6, 4), 0).tolist() == [[255] * 6] * 4
    with pytest.raises(ValueError):
        feather_mask(8, -1)


def host_cases():
    """one frame with eight rows per case: three crop sizes x seven frames (1 x 1 and 2 x 2 up to 131 x 7, the five formats) x two
    passes; scale 0.3 ... 3, +-45 degrees, partly outside (align_tensor_cases.similarities), wholly outside, a NaN, d == 0"""
    buf, frames = C.place(C.FRAMES, 5)
    cases = []
    for rep, (cw, ch), (i, f) in itertools.product(range(2), K.CROPS, enumerate(frames)):
        k = len(cases)
        dtype, layout, channels, order = COMBOS[(5 * k + rep) % len(COMBOS)]
        mats = [S.astype(f32) for S in K.similarities(frames, [i] * 4, cw, ch, 100 + k)] + C.special_matrices(f, cw, ch)
        mode = k % 3
        x = C.tensor(len(mats), cw, ch, dtype, layout, channels, 200 + k)
        alpha = None if mode == 0 else C.alpha_maps(1 if mode == 1 else len(mats), cw, ch, 300 + k, zero_band=k % 2 == 1)
        cases.append(dict(f=f, cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order, gray_shift=14 + k % 2, mats=mats,
                          x=x, alpha=alpha, mode=mode, frame=buf[f["off"]:f["off"] + C.owned_bytes(f)].copy()))
    return cases


def test_host_build_of_the_pixel_code_under_sanitizers(tmp_path):
    exe = B.host_program("align_paste_host", tmp_path)
    cases = host_cases()
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        f = c["f"]
        a = b"" if c["alpha"] is None else c["alpha"].tobytes()
        blob.append(struct.pack("<13i", f["fmt"], f["w"], f["h"], f["stride"], c["cw"], c["ch"], _lib.ALIGN_DTYPES[c["dtype"]],
                                _lib.ALIGN_LAYOUTS[c["layout"]], c["channels"], _lib.ALIGN_ORDERS[c["order"]], c["gray_shift"], len(c["mats"]),
                                c["mode"])
                    + C.SCALES.tobytes() + C.BIASES.tobytes() + b"".join(m.tobytes() for m in c["mats"])
                    + struct.pack("<i", c["x"].nbytes) + c["x"].tobytes() + struct.pack("<i", len(a)) + a
                    + struct.pack("<i", c["frame"].size) + c["frame"].tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 120, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at, seen, touched, formats = 0, 0, 0, set()
    for k, c in enumerate(cases):
        f, n = c["f"], len(c["mats"])
        flags = got[at:at + 4 * n].view(np.int32); at += 4 * n
        W = got[at:at + 24 * n].view(np.uint32).reshape(n, 6); at += 24 * n
        box = got[at:at + 16 * n].view(np.int32).reshape(n, 4); at += 16 * n
        frame = got[at:at + c["frame"].size]; at += c["frame"].size
        want = c["frame"].copy()
        pix = C.view(want, dict(f, off=0))
        rows = [(m, c["x"][r], None if c["alpha"] is None else c["alpha"][r if c["mode"] == 2 else 0]) for r, m in enumerate(c["mats"])]
        res = P.paste(pix, f["fmt"], rows, layout=c["layout"], channels=c["channels"], order=c["order"], scale=C.SCALES, bias=C.BIASES,
                      gray_shift=c["gray_shift"])
        for r, m in enumerate(c["mats"]):
            assert flags[r] == P.flags_at(m, c["cw"], c["ch"], f["w"], f["h"]), (k, r)
            foot = res[r][0]
            if flags[r] & A.DEGENERATE:
                assert not foot.any() and box[r].tolist() == [0, 0, 0, 0]
                continue
            assert np.array_equal(W[r], P.inverse(m)[0].view(np.uint32)), (k, r)
            ys, xs = np.nonzero(foot)
            if ys.size:                                                      # the box holds the footprint
                assert box[r, 0] <= xs.min() and xs.max() < box[r, 2] and box[r, 1] <= ys.min() and ys.max() < box[r, 3], (k, r)
            assert 0 <= box[r, 0] <= box[r, 2] <= f["w"] and 0 <= box[r, 1] <= box[r, 3] <= f["h"]
        assert np.array_equal(frame, want), (k, f, c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"])
        seen |= int(flags.max()) | (int(flags.min() == 0) << 8)
        touched += int((want != c["frame"]).sum())
        formats.add(f["fmt"])
    assert at == got.size
    assert seen == 0x100 | A.DEGENERATE | A.PARTIAL and touched > 10000 and formats == {T.GRAY, T.BGR, T.RGB, T.BGRA, T.RGBA}
