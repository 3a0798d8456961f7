"""The destination frames, tensors and opacity maps that tests/test_gpu_align_paste.py pastes on the device and
tests/test_align_paste_host.py through the host build of the kernel's per-pixel code: frames cut from ONE noise buffer as
align_tensor_cases.place lays them out (odd pitches, misalignment 0-3), 16 guard bytes around each, and its similarities."""
import numpy as np

import align_tensor_cases as K
import align_tensor_ref as T
import paste_ref as P

f32 = np.float32
# (width, height, format): ragged sizes, the five formats a paste can write
FRAMES = [(37, 29, T.BGR), (64, 48, T.RGBA), (5, 4, T.GRAY), (2, 2, T.RGB), (131, 7, T.BGRA), (1, 1, T.GRAY), (33, 21, T.GRAY)]
SCALES = np.array([58.395, 57.12, 57.375], f32)          # the INVERSE of the crop call's: std and mean in 0-255 units
BIASES = np.array([123.675, 116.28, 103.53], f32)
NP_DTYPES = {"uint8": np.uint8, "float16": np.float16, "float32": np.float32}


def place(specs, seed):
    """align_tensor_cases.place with at least 16 bytes between the frames and at both ends; off % 4 == i % 4 stays"""
    _, frames = K.place(specs, seed)
    at = 0
    for i, f in enumerate(frames):
        f["off"] = (at + 16 + 3) // 4 * 4 + i % 4
        at = f["off"] + f["h"] * f["stride"]
    return np.random.default_rng(seed).integers(0, 256, at + 16, dtype=np.uint8), frames


def view(buf, f):
    """the frame's pixels inside buf, writable: h x w x bpp"""
    bpp = P.BPP[f["fmt"]]
    return np.lib.stride_tricks.as_strided(buf[f["off"]:], (f["h"], f["w"], bpp), (f["stride"], bpp, 1))


def owned_bytes(f):
    return (f["h"] - 1) * f["stride"] + f["w"] * P.BPP[f["fmt"]]


def tensor(n, cw, ch, dtype, layout, channels, seed, scale=SCALES, bias=BIASES):
    """N rows of a network's output: decoded values spread over -40 ... 295 (so both clamps act), and -- float dtypes -- a NaN, an
    infinity of each sign in every row"""
    rng = np.random.default_rng(seed)
    shape = (n, channels, ch, cw) if layout == "nchw" else (n, ch, cw, channels)
    if dtype == "uint8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    val = rng.uniform(-40.0, 295.0, shape)
    s, b = np.asarray(scale, np.float64)[:channels], np.asarray(bias, np.float64)[:channels]
    bc = (1, channels, 1, 1) if layout == "nchw" else (1, 1, 1, channels)
    x = ((val - b.reshape(bc)) / s.reshape(bc)).astype(NP_DTYPES[dtype])
    flat = x.reshape(n, -1)
    for r in range(n):
        at = rng.choice(flat.shape[1], min(3, flat.shape[1]), replace=False)
        flat[r, at] = np.array([np.nan, np.inf, -np.inf], flat.dtype)[:at.size]
    return x


def alpha_maps(n, cw, ch, seed, zero_band=False):
    """n random opacity maps; zero_band: the left half of every map is 0"""
    a = np.random.default_rng(seed).integers(0, 256, (n, ch, cw), dtype=np.uint8)
    a[:, 0, 0] = 255
    if zero_band:
        a[:, :, :max(1, cw // 2)] = 0
    return a


def special_matrices(f, cw, ch):
    """crop -> frame matrices beyond align_tensor_cases.similarities: wholly outside the frame, a NaN, d == 0, exactly the identity"""
    return [np.array([[1, 0, f["w"] + 40.0], [0, 1, -3.0 * ch - 40.0]], f32), np.array([[1, 0, np.nan], [0, 1, 0]], f32),
            np.array([[1, 2, 3], [2, 4, 1]], f32), np.array([[1, 0, 0], [0, 1, 0]], f32)]
