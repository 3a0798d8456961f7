"""The YUV frame sets of tests/test_yuv_host.py and tests/test_gpu_yuv_*.py (include/sdm.h, "YUV colour description and 10-bit
surfaces"): NV12 and P010 frames of planar_cases' kind cut from ONE noise buffer -- 1 x 1, 2 x 2, 5 x 4, 37 x 29, 38 x 34 and 64 x 48,
odd pitches (even for P010, whose pointers and strides must be), the UV plane both directly behind the luma and apart from it.  A frame
is described as align_tensor_cases.place describes it, plus `name` (base[:matrix][:range]) and `desc` (yuv_ref.Desc)."""
import numpy as np

import align_tensor_cases as K
import align_tensor_ref as T
import yuv_ref as Y

SIZES = [(1, 1), (2, 2), (5, 4), (37, 29), (38, 34), (64, 48)]
NAMES8 = ["nv12:" + m + (":full" if full else "") for m, full in Y.DESCRIPTIONS]          # "nv12:bt601" is value 5
NAMES10 = ["p010:" + m + (":full" if full else "") for m, full in Y.DESCRIPTIONS]


def place(specs, seed=23):
    """specs: (width, height, name, pitch padding in bytes, UV apart).  (noise buffer uint8, frames): frame i = dict(name, desc, fmt, w, h,
    stride, off, uv_off, separate); fmt is T.NV12 for an 8-bit frame, "p010" for a 10-bit one; a BGR entry (name "bgr") rides along as
    align_tensor_cases places it"""
    rng = np.random.default_rng(seed)
    frames, at = [], 16
    for i, (w, h, name, pad, apart) in enumerate(specs):
        if name == "bgr":
            stride, start = 3 * w + pad, (at + 3) // 4 * 4 + i % 4
            frames.append(dict(name=name, desc=None, fmt=T.BGR, w=w, h=h, stride=stride, off=start, uv_off=None, separate=False))
            at = start + h * stride
            continue
        desc = Y.Desc(name)
        ten = desc.base == "p010"
        bps = 2 if ten else 1
        stride = max(w * bps, 2 * bps * ((w + 1) // 2)) + pad
        start = (at + 3) // 4 * 4 + (2 * (i % 2) if ten else i % 4)
        assert not ten or (stride % 2 == 0 and start % 2 == 0)
        uv_off = start + h * stride + (38 if apart else 0)
        frames.append(dict(name=name, desc=desc, fmt="p010" if ten else T.NV12, w=w, h=h, stride=stride, off=start, uv_off=uv_off,
                           separate=apart))
        at = uv_off + ((h + 1) // 2) * stride
    return rng.integers(0, 256, at + 64, dtype=np.uint8), frames


def words(buf, off, shape, stride):
    """a plane of 16-bit little-endian words in buf as uint16 (copy): shape = (rows, words per row), stride in bytes"""
    rows, n = shape
    b = np.lib.stride_tricks.as_strided(buf[off:], (rows, 2 * n), (stride, 1)).astype(np.uint16)
    return b[:, 0::2] | (b[:, 1::2] << 8)


def host_frame(buf, f):
    """align_tensor_ref.Frame of an 8-bit frame (its description is f["desc"]), yuv_ref.Frame10 of a P010 one (copies)"""
    if f["fmt"] != "p010":
        return K.host_frame(buf, f)
    w, h = f["w"], f["h"]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return Y.Frame10(f["desc"], words(buf, f["off"], (h, w), f["stride"]), words(buf, f["uv_off"], (ch, 2 * cw), f["stride"]).reshape(ch, cw, 2))


def plane_bytes(f):
    """(bytes of plane 0, bytes of the UV plane) the frame owns: up to the last element of the last row"""
    bps = 2 if f["fmt"] == "p010" else 1
    return (f["h"] - 1) * f["stride"] + bps * f["w"], ((f["h"] + 1) // 2 - 1) * f["stride"] + 2 * bps * ((f["w"] + 1) // 2)


def owned(f):
    """byte offsets into the buffer that the frame's samples occupy"""
    if f["fmt"] == T.BGR:
        return (np.arange(f["h"])[:, None] * f["stride"] + np.arange(3 * f["w"])[None, :]).reshape(-1) + f["off"]
    bps = 2 if f["fmt"] == "p010" else 1
    y = (np.arange(f["h"])[:, None] * f["stride"] + np.arange(bps * f["w"])[None, :]).reshape(-1) + f["off"]
    uv = (np.arange((f["h"] + 1) // 2)[:, None] * f["stride"] + np.arange(2 * bps * ((f["w"] + 1) // 2))[None, :]).reshape(-1) + f["uv_off"]
    return np.concatenate([y, uv])


def device_frames(dev, frames):
    """(the frame list, chroma) a ``frames=`` call takes for the buffer `dev` (a uint8 device tensor): every frame a tuple named by its
    description, a UV plane that lies apart in `chroma`"""
    base = dev.data_ptr()
    lst = [(base + f["off"], f["w"], f["h"], f["stride"], f["name"]) for f in frames]
    return lst, [base + f["uv_off"] if f["separate"] else None for f in frames]
