"""The frame sets that tests/test_gpu_align_tensor.py runs on the device and tests/test_align_tensor_host.py runs through the host build
of the kernel's per-pixel code: views cut from ONE noise buffer -- odd pitches, source misalignment 0-3 -- and known similarities."""
import numpy as np

import align_ref as A
import align_tensor_ref as T

BPP = {T.GRAY: 1, T.NV12: 1, T.BGR: 3, T.RGB: 3, T.BGRA: 4, T.RGBA: 4}
NAMES = {T.GRAY: "gray", T.BGR: "bgr", T.RGB: "rgb", T.BGRA: "bgra", T.RGBA: "rgba", T.NV12: "nv12"}
# (width, height, format): ragged sizes, all six formats
RAGGED = [(37, 29, T.BGR), (64, 48, T.RGBA), (5, 4, T.NV12), (2, 2, T.RGB), (131, 7, T.BGRA), (1, 1, T.GRAY)]
# even and odd width and height; the bool: the UV plane at a pointer of its own (with the luma's stride) instead of behind the luma
NV12 = [(6, 4, T.NV12, False), (7, 5, T.NV12, True), (1, 1, T.NV12, False), (6, 4, T.NV12, True)]
CROPS = [(5, 3), (7, 7), (16, 16)]


def place(specs, seed):
    """(noise buffer uint8, frames): frame i = dict(fmt, w, h, stride, off, uv_off) with off % 4 == i % 4 and an odd pitch padding"""
    rng = np.random.default_rng(seed)
    frames, at = [], 16
    for i, spec in enumerate(specs):
        w, h, fmt = spec[:3]
        separate = len(spec) > 3 and spec[3]
        row = max(w * BPP[fmt], 2 * ((w + 1) // 2)) if fmt == T.NV12 else w * BPP[fmt]
        stride = row + 2 * i + 1
        off = (at + 3) // 4 * 4 + i % 4
        at = off + h * stride
        f = dict(fmt=fmt, w=w, h=h, stride=stride, off=off, uv_off=None)
        if fmt == T.NV12:
            ch = (h + 1) // 2
            f["uv_off"] = at + 37 if separate else off + h * stride
            f["separate"] = separate
            at = f["uv_off"] + ch * stride
        frames.append(f)
    return rng.integers(0, 256, at + 64, dtype=np.uint8), frames


def plane_bytes(f):
    """(bytes of plane 0, bytes of the UV plane) a reader may touch: up to the last pixel of the last row"""
    b0 = (f["h"] - 1) * f["stride"] + f["w"] * BPP[f["fmt"]]
    b1 = ((f["h"] + 1) // 2 - 1) * f["stride"] + 2 * ((f["w"] + 1) // 2) if f["fmt"] == T.NV12 else 0
    return b0, b1


def host_frame(buf, f):
    """the frame's pixels as align_tensor_ref.Frame (copies)"""
    w, h, s, bpp = f["w"], f["h"], f["stride"], BPP[f["fmt"]]
    st = np.lib.stride_tricks.as_strided
    pix = st(buf[f["off"]:], (h, w, bpp), (s, bpp, 1)).copy()
    uv = None
    if f["fmt"] == T.NV12:
        uv = st(buf[f["uv_off"]:], ((h + 1) // 2, (w + 1) // 2, 2), (s, 2, 1)).copy()
    return T.Frame(f["fmt"], pix[..., 0] if bpp == 1 else pix, uv)


def similarities(frames, rows_to_frames, width, height, seed):
    """one crop -> source similarity per row: scale 0.3 ... 3, +-45 degrees, the crop centre near the frame centre -- borders and
    PARTIAL occur"""
    rng = np.random.default_rng(seed)
    out = []
    for r, im in enumerate(rows_to_frames):
        f = frames[im]
        s = [0.3, 3.0, 1.0][r % 3] if r < 3 else rng.uniform(0.3, 3.0)
        a = [45.0, -45.0, 0.0][r % 3] if r < 3 else rng.uniform(-45, 45)
        S = A.similarity(s * max(f["w"], f["h"]) / max(width, height), a, 0, 0)
        c = np.array([(width - 1) / 2, (height - 1) / 2])
        S[:, 2] = np.array([(f["w"] - 1) / 2, (f["h"] - 1) / 2]) + rng.uniform(-0.3, 0.3, 2) * (f["w"], f["h"]) - S[:, :2] @ c
        out.append(S)
    return out


def landmark_rows(sims, template, landmark_index, L):
    """rows x (N x 2L float32) whose selected landmarks are the template points seen through each row's similarity"""
    x = np.zeros((len(sims), 2 * L), np.float32)
    for r, S in enumerate(sims):
        p = A.apply(S, template)
        x[r, np.asarray(landmark_index)] = p[:, 0]
        x[r, L + np.asarray(landmark_index)] = p[:, 1]
    return x
