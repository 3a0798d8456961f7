"""The frame sets, rows and meshes of tests/test_gpu_warp.py, tests/test_warp_host.py and tests/test_cpp_warp.py: four frames of four
formats cut from ONE noise buffer at odd pitches and source misalignments 0-3, six rows over them, and three meshes."""
import numpy as np

import align_tensor_cases as K
import align_tensor_ref as T
from superviseddescent_amd import alignment_template, delaunay, ibug

IDS = ibug.RCR22_IDS
L = len(IDS)
MEAN = ibug.select_mean(IDS)
# (width, height, format, stride): gray at pitch 41, BGR at pitch 113, RGBA dense, NV12 with a chroma plane of its own
FRAMES = [(40, 36, T.GRAY, 41), (37, 33, T.BGR, 113), (48, 40, T.RGBA, 192), (38, 34, T.NV12, 39)]
ROWS = [0, 1, 2, 3, 1, 3]                       # row -> frame
CROPS = [(24, 20), (33, 17)]


def place(seed=5):
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


def mesh_rcr22(w, h):
    """(landmark indices, template, triangles): all 22 landmarks, the default template and its Delaunay triangulation"""
    idx = np.arange(L)
    t = alignment_template(MEAN, idx, w, h, 0.1)
    return idx, t, delaunay(t)


def mesh_single(w, h):
    return np.array([2, 7, 11]), np.array([[1.0, 1.0], [w - 2.0, 2.0], [w / 2.0, h - 1.5]], np.float32), np.array([[0, 1, 2]], np.int32)


def mesh_254(w, h):
    """254 triangles by cycling the Delaunay list (and turning every second round over): the LDS bound"""
    idx, t, tri = mesh_rcr22(w, h)
    reps = [tri if r % 2 == 0 else tri[:, [0, 2, 1]] for r in range(254 // len(tri) + 1)]
    return idx, t, np.concatenate(reps)[:254].astype(np.int32)


def rows_for(frames, rows_to_frames, idx, template, w, h, seed, bend=0.02, L=L):
    """N x 2L float32 rows whose mesh landmarks are the template, sheared and bent a little (no longer a similarity; gentle enough that
    not even the mesh's slivers fold), seen through a similarity into the row's frame: scale, rotation and offset vary, and some rows
    reach over the border."""
    rng = np.random.default_rng(seed)
    sims = K.similarities(frames, rows_to_frames, w, h, seed)
    x = rng.uniform(0, 30, (len(sims), 2 * L)).astype(np.float32)          # (landmarks outside the mesh: any finite value)
    c = np.array([(w - 1) / 2, (h - 1) / 2])
    for r, S in enumerate(sims):
        S = S.copy()
        S[:, :2] *= 0.6                                                    # (most of the face inside the frame)
        f = frames[rows_to_frames[r]]
        S[:, 2] = np.array([(f["w"] - 1) / 2, (f["h"] - 1) / 2]) - S[:, :2] @ c + rng.uniform(-3, 3, 2)
        d = np.asarray(template, np.float64) - c
        shear = np.array([[1 + rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)], [rng.uniform(-0.2, 0.2), 1 + rng.uniform(-0.2, 0.2)]])
        q = d @ shear.T + bend * np.stack([d[:, 1] ** 2 / h, d[:, 0] ** 2 / w], 1) * rng.choice([-1, 1], 2) + c
        p = q @ S[:, :2].T + S[:, 2]
        x[r, np.asarray(idx)] = p[:, 0]
        x[r, L + np.asarray(idx)] = p[:, 1]
    return x
