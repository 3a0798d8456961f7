"""The planar colour frame sets of tests/test_gpu_planar_frames.py and tests/test_gpu_planar_paste.py (include/sdm.h, "Planar colour
frames"): frames cut from ONE noise buffer -- odd pitches, source misalignment 0-3, the planes at the default distance, at a padded odd
one, 64 bytes further and at a negative one --, a region view of a larger 3 x H x W block, and a BGR and an NV12 frame beside them.  A
frame is described as align_tensor_cases.place describes it, plus `D`, the plane distance in bytes; the expected values come from the
references of the interleaved formats, applied to the interleaved view of the same pixels (host_frame)."""
import numpy as np

import align_tensor_cases as K
import align_tensor_ref as T

BGR_PLANAR, RGB_PLANAR = 16, 17
NAMES = {**K.NAMES, BGR_PLANAR: "bgr_planar", RGB_PLANAR: "rgb_planar"}
PACKED = {BGR_PLANAR: T.BGR, RGB_PLANAR: T.RGB}                     # the interleaved format of the same bytes
# (width, height, format, pitch padding, plane distance: "default" | "odd" (default + 3) | "far" (default + 64) | "negative")
FRAMES = [(37, 29, BGR_PLANAR, 1, "default"), (64, 48, RGB_PLANAR, 3, "odd"), (5, 4, BGR_PLANAR, 0, "negative"),
          (2, 2, RGB_PLANAR, 5, "far"), (1, 1, BGR_PLANAR, 0, "default"), (41, 33, RGB_PLANAR, 39, "region"),
          (37, 29, T.BGR, 2, None), (38, 34, T.NV12, 1, None)]


def is_planar(f):
    return f["fmt"] in PACKED


def place(specs=FRAMES, seed=17):
    """(noise buffer uint8, frames): frame i = dict(fmt, w, h, stride, off, uv_off, D) with off % 4 == i % 4.  "region": the frame is
    x[:, 10:10 + h, 20:20 + w] of a 3 x (h + 27) x (w + pad) block -- its planes are a whole block plane apart"""
    rng = np.random.default_rng(seed)
    frames, at = [], 16
    for i, (w, h, fmt, pad, kind) in enumerate(specs):
        stride = (max(w, 2 * ((w + 1) // 2)) if fmt == T.NV12 else w * K.BPP.get(fmt, 1)) + pad
        start = (at + 3) // 4 * 4 + i % 4
        f = dict(fmt=fmt, w=w, h=h, stride=stride, off=start, uv_off=None, D=None, kind=kind)
        if fmt in PACKED:
            gap = {"default": h * stride, "odd": h * stride + 3, "far": h * stride + 64, "negative": h * stride + 5,
                   "region": (h + 27) * stride}[kind]
            f["D"] = -gap if kind == "negative" else gap
            if kind == "negative":
                f["off"] = start + 2 * gap                          # data is the HIGHEST plane
            if kind == "region":
                f["off"] = start + 10 * stride + 20
                at = start + 3 * gap
            else:
                at = start + 2 * gap + h * stride
        elif fmt == T.NV12:
            f["uv_off"], f["separate"] = start + h * stride + 37, True
            at = f["uv_off"] + ((h + 1) // 2) * stride
        else:
            at = start + h * stride
        frames.append(f)
    return rng.integers(0, 256, at + 64, dtype=np.uint8), frames


def planes(buf, f):
    """the three planes of a planar frame as views into buf, in the order they lie in memory by plane index: (3, h, w)"""
    st = np.lib.stride_tricks.as_strided
    return np.stack([st(buf[f["off"] + c * f["D"]:], (f["h"], f["w"]), (f["stride"], 1)) for c in range(3)])


def host_frame(buf, f):
    """align_tensor_ref.Frame of the frame's pixels (copies): a planar frame as the interleaved frame of the same three bytes"""
    if not is_planar(f):
        return K.host_frame(buf, f)
    return T.Frame(PACKED[f["fmt"]], np.ascontiguousarray(np.transpose(planes(buf, f), (1, 2, 0))), None)


def owned(f):
    """byte offsets into the buffer that the frame's pixels occupy (every plane, up to the last pixel of every row)"""
    rows = np.arange(f["h"])[:, None] * f["stride"]
    if is_planar(f):
        one = (rows + np.arange(f["w"])[None, :]).reshape(-1)
        return np.concatenate([f["off"] + c * f["D"] + one for c in range(3)])
    one = (rows + np.arange(f["w"] * K.BPP[f["fmt"]])[None, :]).reshape(-1) + f["off"]
    if f["fmt"] == T.NV12:
        uv = (np.arange((f["h"] + 1) // 2)[:, None] * f["stride"] + np.arange(2 * ((f["w"] + 1) // 2))[None, :]).reshape(-1) + f["uv_off"]
        one = np.concatenate([one, uv])
    return one


def device_frames(dev, frames):
    """(the frame list, formats, chroma) a ``frames=`` call takes for the buffer `dev` (a uint8 device tensor): planar frames with a
    positive plane distance as 3 x H x W VIEWS named by `formats` -- their second plane comes from the view's strides --, the one with a
    negative distance as a tuple with its second plane in `chroma`, BGR as a tensor view, NV12 as a tuple with its UV plane"""
    import torch
    base = dev.data_ptr()
    lst, formats, chroma = [], [], []
    for f in frames:
        name = NAMES[f["fmt"]]
        if is_planar(f) and f["D"] > 0:
            lst.append(torch.as_strided(dev, (3, f["h"], f["w"]), (f["D"], f["stride"], 1), f["off"]))
            formats.append(name)
            chroma.append(None)
        elif is_planar(f):
            lst.append((base + f["off"], f["w"], f["h"], f["stride"], name))
            formats.append(None)
            chroma.append(base + f["off"] + f["D"])
        elif f["fmt"] == T.NV12:
            lst.append((base + f["off"], f["w"], f["h"], f["stride"], name))
            formats.append(None)
            chroma.append(base + f["uv_off"])
        else:
            bpp = K.BPP[f["fmt"]]
            shape, stride = ((f["h"], f["w"]), (f["stride"], 1)) if bpp == 1 else ((f["h"], f["w"], bpp), (f["stride"], bpp, 1))
            lst.append(torch.as_strided(dev, shape, stride, f["off"]))
            formats.append(name)
            chroma.append(None)
    return lst, formats, chroma
