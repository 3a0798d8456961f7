"""The frames, rows and meshes of the filtered warp's tests (tests/test_warp_area_host.py, tests/test_gpu_warp_area.py,
tests/test_cpp_warp_area.py).  The frames of tests/warp_cases.py are 37-48 pixels wide and cannot hold a row that minifies, so: four
frames of the same four formats at awkward pitches, 128-150 pixels wide, cut from ONE noise buffer at source misalignments 0-3; the crops
and the meshes of warp_cases; six rows whose crop -> source scale runs from below 1 to about 5, sheared and bent so that the triangles
of one face ask for different and anisotropic (Sx, Sy).  tests/test_warp_area_host.py asserts what the set must cover."""
import numpy as np

import align_ref as A
import align_tensor_ref as T
import warp_cases as W

IDS, L, MEAN = W.IDS, W.L, W.MEAN
# (width, height, format, stride): gray at pitch 133, BGR at pitch 457, RGBA at pitch 516, NV12 (pitch 143) with a chroma plane of its own
FRAMES = [(131, 113, T.GRAY, 133), (150, 97, T.BGR, 457), (128, 120, T.RGBA, 516), (142, 110, T.NV12, 143)]
ROWS = [0, 1, 2, 3, 1, 3]                       # row -> frame
CROPS = W.CROPS
MESHES = {"rcr22": W.mesh_rcr22, "single": W.mesh_single, "254": W.mesh_254}
# per row: the similarity's scale in units of min(frame w / crop w, frame h / crop h) / 4.6, the weight of the shear, the crop centre's
# offset from the frame's centre in frame widths / heights.  Row 0 magnifies (every triangle at (1, 1)); row 3 reaches over the border.
SCALES = [0.6, 1.7, 2.6, 4.2, 3.3, 2.1]
SHEAR = [0.2, 1.0, 1.0, 0.6, 1.0, 1.0]
OFFSET = [(0, 0), (0.02, -0.03), (-0.03, 0.02), (0.42, 0.1), (0.01, 0.04), (-0.02, -0.02)]
SEED = 21                                       # the rows of the shared case set: rows_for(..., SEED)


def place(seed=6):
    """(noise buffer, frames as align_tensor_cases.place describes them): frame i starts at an address with off % 4 == i"""
    rng = np.random.default_rng(seed)
    frames, at = [], 16
    for i, (w, h, fmt, stride) in enumerate(FRAMES):
        off = (at + 3) // 4 * 4 + i % 4
        at = off + h * stride
        f = dict(fmt=fmt, w=w, h=h, stride=stride, off=off, uv_off=None)
        if fmt == T.NV12:
            f["uv_off"], f["separate"] = at + 37, True
            at = f["uv_off"] + ((h + 1) // 2) * stride
        frames.append(f)
    return rng.integers(0, 256, at + 64, dtype=np.uint8), frames


def rows_for(frames, rows_to_frames, idx, template, w, h, seed, bend=0.02, scales=SCALES, L=L):
    """N x 2L float32 rows whose mesh landmarks are the template, sheared (+-0.3 along the axes, +-0.2 across) and bent (no longer a
    similarity, and gentle enough that nothing folds), seen through a similarity of the row's scale into the row's frame"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 30, (len(rows_to_frames), 2 * L)).astype(np.float32)          # (landmarks outside the mesh: any finite value)
    c = np.array([(w - 1) / 2, (h - 1) / 2])
    for r, im in enumerate(rows_to_frames):
        f = frames[im]
        s = scales[r % len(scales)] * min(f["w"] / w, f["h"] / h) / 4.6
        S = A.similarity(s, rng.uniform(-25, 25), 0, 0)
        centre = np.array([(f["w"] - 1) / 2, (f["h"] - 1) / 2]) + np.array(OFFSET[r % len(OFFSET)]) * (f["w"], f["h"]) + rng.uniform(-2, 2, 2)
        S[:, 2] = centre - S[:, :2] @ c
        k = SHEAR[r % len(SHEAR)]
        shear = np.array([[1 + k * rng.uniform(-0.3, 0.3), k * rng.uniform(-0.2, 0.2)], [k * rng.uniform(-0.2, 0.2), 1 + k * rng.uniform(-0.3, 0.3)]])
        d = np.asarray(template, np.float64) - c
        q = d @ shear.T + bend * np.stack([d[:, 1] ** 2 / h, d[:, 0] ** 2 / w], 1) * rng.choice([-1, 1], 2) + c
        p = A.apply(S, q)
        x[r, np.asarray(idx)] = p[:, 0]
        x[r, L + np.asarray(idx)] = p[:, 1]
    return x
