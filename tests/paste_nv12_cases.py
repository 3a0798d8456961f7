"""The destination frames, rows, tensors and opacity maps of the paste into NV12 frames (include/sdm.h, "Pasting crops back into NV12
frames") that tests/test_align_paste_nv12_host.py runs through the host build of the block code and tests/test_gpu_align_paste_nv12.py on
the device.  Every plane is cut from ONE noise buffer as paste_cases.place does it: 16 guard bytes around each plane, odd pitches, plane
starts misaligned by 0-3.  Odd width, odd height, both, a single pixel, wide and flat; the UV plane directly behind Y (``chroma`` None) or
elsewhere in the buffer at a misalignment of its own; one BGR and one GRAY frame in the same list."""
import numpy as np

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import paste_area_cases as D
import paste_area_ref as Q
import paste_cases as C
import paste_nv12_ref as N
import paste_ref as P

f32 = np.float32
# (width, height, format, the UV plane at a place of its own)
FRAMES = [(37, 29, T.NV12, False), (64, 48, T.NV12, True), (5, 4, T.NV12, True), (2, 2, T.NV12, False), (1, 1, T.NV12, True),
          (131, 7, T.NV12, False), (33, 21, T.NV12, True), (37, 29, T.BGR, False), (33, 21, T.GRAY, False)]
NV12_FRAMES = 7
CROPS = [(16, 16), (7, 5), (33, 20)]
# (dtype, layout, channels, order): u8, f16 and f32; both layouts; three channels in both orders and one channel
COMBOS = [("uint8", "nhwc", 3, "bgr"), ("float16", "nchw", 3, "rgb"), ("float32", "nhwc", 1, "bgr"), ("float16", "nhwc", 3, "bgr"),
          ("float32", "nchw", 3, "rgb"), ("uint8", "nchw", 1, "rgb")]
# None: plain bilinear; else (mode, max_samples, min_scale)
FILTERS = [None, (Q.AREA, 16, 1.0), None, (Q.AREA, 16, 1.0), (Q.BILINEAR, 16, 1.0), (Q.AREA, 4, 1.0)]
W_SCALES = [0.8, 1.7, 2.6]                                  # crop pixels per frame pixel: S = 1, 2, 3 under "area"


def place(specs=FRAMES, seed=11):
    """(noise buffer, frames): frame i = dict(fmt, w, h, stride, off, uv_off, separate).  Plane starts: off % 4 == i % 4, a separate UV
    plane at (i + 1) % 4 -- behind ALL luma planes, so that no frame's planes are neighbours --, pitch = row bytes + 2 i + 1 (odd for NV12)"""
    frames, at = [], 0
    for i, (w, h, fmt, separate) in enumerate(specs):
        row = 2 * ((w + 1) // 2) if fmt == T.NV12 else w * P.BPP[fmt]
        stride = row + 2 * i + 1
        off = (at + 16 + 3) // 4 * 4 + i % 4
        at = off + h * stride
        f = dict(fmt=fmt, w=w, h=h, stride=stride, off=off, uv_off=None, separate=separate)
        if fmt == T.NV12 and not separate:
            f["uv_off"] = at
            at += (h + 1) // 2 * stride
        frames.append(f)
    for i, f in enumerate(frames):
        if f["fmt"] == T.NV12 and f["separate"]:
            f["uv_off"] = (at + 16 + 3) // 4 * 4 + (i + 1) % 4
            at = f["uv_off"] + (f["h"] + 1) // 2 * f["stride"]
    return np.random.default_rng(seed).integers(0, 256, at + 16, dtype=np.uint8), frames


def planes(buf, f):
    """the NV12 frame's planes inside buf, writable: (Y h x w, UV ceil(h/2) x ceil(w/2) x 2)"""
    st = np.lib.stride_tricks.as_strided
    return (st(buf[f["off"]:], (f["h"], f["w"]), (f["stride"], 1)),
            st(buf[f["uv_off"]:], ((f["h"] + 1) // 2, (f["w"] + 1) // 2, 2), (f["stride"], 2, 1)))


def owned_bytes(f):
    """(bytes of the Y plane, bytes of the UV plane) up to the last byte of the last row"""
    return (f["h"] - 1) * f["stride"] + f["w"], ((f["h"] + 1) // 2 - 1) * f["stride"] + 2 * ((f["w"] + 1) // 2)


def rows_of(frames, cw, ch, seed, filtered):
    """(matrices, frame of every row).  Frame 0: three overlapping similarities (scale 0.3, 3 and 1 of align_tensor_cases: the first at
    45 degrees, its edge cuts blocks in half) and an integer translation to ODD coordinates, whose edges cut every block they meet; then the
    special matrices -- wholly outside, a NaN, d == 0, the identity.  Frame 1: three rows of W scale 0.8, 1.7, 2.6 (S = 1, 2, 3 when
    filtered), overlapping; two overlapping rows on frame 6; one row on every other frame, BGR and GRAY included."""
    idx = [0, 0, 0]
    mats = [S.astype(f32) for S in K.similarities(frames, idx, cw, ch, seed)]
    mats.append(np.array([[1, 0, 3], [0, 1, 1]], f32))
    idx.append(0)
    for m in C.special_matrices(frames[0], cw, ch):
        mats.append(m)
        idx.append(0)
    centre = np.array([(cw - 1) / 2.0, (ch - 1) / 2.0])
    for r, s in enumerate(W_SCALES):
        R = A.similarity(1.0 / s, 20.0 * r - 15.0, 0.0, 0.0)[:, :2]
        t = np.array([30.0 + 3 * r, 22.0 + 2 * r]) - R @ centre
        mats.append(np.concatenate([R, t[:, None]], 1).astype(f32))
        idx.append(1)
    for i in (2, 3, 4, 5, 6, 6, 7, 8):
        mats.append(K.similarities(frames, [i] * 4, cw, ch, seed + i)[3 if filtered else 2].astype(f32))
        idx.append(i)
    return np.stack(mats), idx


def calls():
    """one call per combination: the frame list of place(), a crop size, a tensor, an opacity map (none, shared, per row; with a zero
    band in turn) and a filter"""
    buf, frames = place()
    out = []
    for k, (dtype, layout, channels, order) in enumerate(COMBOS):
        cw, ch = CROPS[k % 3]
        filt = FILTERS[k]
        mats, idx = rows_of(frames, cw, ch, 900 + 10 * k, filt is not None)
        x = C.tensor(len(idx), cw, ch, dtype, layout, channels, 40 + k)
        alpha = [None, C.alpha_maps(1, cw, ch, 50 + k, zero_band=k == 4)[0], C.alpha_maps(len(idx), cw, ch, 60 + k, zero_band=k == 2)][k % 3]
        out.append(dict(buf=buf, frames=frames, cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order,
                        gray_shift=14 if order == "bgr" else 15, mats=mats, idx=idx, x=x, alpha=alpha, filter=filt))
    return out


def spec_of(c):
    return dict(layout=c["layout"], order=c["order"], scale=C.SCALES, bias=C.BIASES, gray_shift=c["gray_shift"])


def alpha_of(c, r):
    return None if c["alpha"] is None else c["alpha"] if c["alpha"].ndim == 2 else c["alpha"][r]


def expect(c):
    """(the restatement on a copy of the buffer: every frame's rows in row order, S of every row, the luma pixels with an opacity above 0
    per frame, the chroma samples written per frame)"""
    want, S = c["buf"].copy(), []
    spec, filt = spec_of(c), c["filter"]
    for r, im in enumerate(c["idx"]):
        f, m = c["frames"][im], c["mats"][r]
        degenerate = P.inverse(m)[1]
        S.append(1 if filt is None or degenerate else Q.samples(m, *filt))
        if degenerate:
            continue
        if f["fmt"] == T.NV12:
            Y, UV = planes(want, f)
            N.paste_row(Y, UV, m, c["x"][r], alpha_of(c, r), S[-1], channels=c["channels"], **spec)
        else:
            Q.paste_row(C.view(want, f), f["fmt"], m, c["x"][r], alpha_of(c, r), S[-1], channels=c["channels"], **spec)
    return want, S
