"""Head-pose cases at every model size the C-ABI takes (1 <= K <= 64 points, up to 16 levels), for tests/test_gpu_pose_shapes.py: the
kernels of csrc/sdm_pose.hip are shaped by K (the Gram kernel's pairs per thread, the cascade's template chunks, the solve's LDS
system) and by the row count (256 rows per cascade block, 64 per projection block, 64-row Gram chunks, partials reduced in eights),
and a model of 13, 33 or 64 points must meet the same code as the example's ten.  Host only: the case table, the inputs, a float32
restatement of one level in numpy (the reference's own float32 noise floor, not the device) and the launchers' LDS sizes and block
counts.  tests/test_pose_cases_host.py checks the conditions the cases must meet.

  points(K)                      the K x 3 model (K = 10: the example's)
  poses(n, seed, limit)          n x 6 parameter rows, angles uniform in +-limit degrees, t = (0, 0, -2000)
  CASES                          (K, T, pairs, kp, instantiation, cascade chunks) for every K of KS
  project32 / update32 / level32 / cascade32    float32 numpy in the kernel's order of operations
  lds_bytes_cascade / lds_bytes_solve / gram_rows / gram_blocks    the launchers' arithmetic
"""
import collections

import numpy as np

import pose_f64 as P

# ---- the kernel's constants (csrc/sdm_pose.hip) ------------------------------------------------------------------------------------
THREADS = 256                 # POSE_THREADS :28: rows per cascade block, pairs per round of the Gram kernel
GRAM_CHUNK = 64               # POSE_GRAM_CHUNK :29
GRAM_BLOCKS = 512             # POSE_GRAM_BLOCKS :30
CHUNK_PTS = 16                # POSE_CHUNK_PTS :33: K <= 16 keeps a block's templates resident, larger K stages 16 points at a time
PROJ_ROWS = 64                # POSE_PROJ_ROWS :34
REDUCE_GROUP = 8              # pose_gram_reduce_kernel :232-237: partials summed in groups of eight blocks, then a tail
GRAM_KP = [2, 4, 8, 16, 36]   # sdm_launch_pose_gram :387-391: the instantiation is the first KP >= kp; 36 = POSE_MAXP :31
MAX_K, MAX_LEVELS = 64, 16    # csrc/sdm_kernels.h: SDM_POSE_MAX_K, SDM_POSE_MAX_LEVELS
CASCADE_LDS_LIMIT = 96 * 1024     # sdm_launch_pose_cascade :362
SOLVE_LDS_LIMIT = 150 * 1024      # sdm_launch_pose_solve :399

# ---- the cases -------------------------------------------------------------------------------------------------------------------------
# both sides of every Gram threshold (12|13, 19|20, 28|29, 42|43), and on both cascade paths (K <= 16 | K > 16) a whole chunk, a
# tail of one point and a tail of 15 or 16
KS = [1, 2, 3, 12, 13, 15, 16, 17, 19, 20, 28, 29, 32, 33, 42, 43, 63, 64]
N_DEFAULT = 321                                       # two cascade blocks (256 + 65), six projection and Gram blocks (5 x 64 + 1)
N_ROWS = [1, 63, 64, 65, 255, 256, 257, 513]          # cascade and projection: around one wave, one block, two blocks
N_GRAM = [1, 64, 65, 129, 576, 32768, 32769]          # training: 1, 1, 2, 3, 9, 512 and 257 Gram blocks
GRAM_BLOCKS_OF = dict(zip(N_GRAM, [1, 1, 2, 3, 9, 512, 257]))
# (reg_type, param, regularise_last_row): Regulariser::RegularisationType Manual = 0, MatrixNorm = 1
REGULARISERS = [(1, 2.0, True), (1, 2.0, False), (0, 1e-3, True), (0, 1e-3, False)]
# the project's bounds on x_{k+1} and on the cascade: of ||x*||, and of the norm of x*'s angles (tests/test_gpu_pose.py)
X_TOL, ANGLE_TOL = 1e-7, 1e-5
FEAT_TOL = 6e-6                                       # float32 projection vs float64, max |error| per row / max |u, v| of the row
R_TOL = 2.0 ** -23                                    # |R_dev - R64| / max |R64|: one float32 rounding of the same float64 system, x 2
COND_CAP = 1e6                                        # a condition on the inputs: cond(G + Lambda) of every system a test solves
# The device's worst case per K as tests/test_gpu_pose_shapes.py measured it on an MI355X, over every level, regulariser and row
# count of the module: (features, R as share of max |R64|, x_{k+1} of ||x*||, of the angles' norm, cascade of ||x*||, of the angles'
# norm).  R never used more than 0.44 of R_TOL (one float32 rounding is half of it), x_{k+1} and the cascade never more than 0.26 of
# their bounds; 257 of the 283 bounds were the project's own, the others four times the restatement's error (K <= 3, single levels
# of the Manual regulariser with the last row free, the cascades of random regressors), the widest 4.5e-7 / 3.0e-5 at K = 1.
DEVICE_MEASURED = {
    1: (3.1e-06, 4.1e-08, 1.1e-07, 7.2e-06, 5.5e-08, 3.6e-06),
    2: (2.9e-06, 4.3e-08, 4.7e-08, 3.2e-06, 4.3e-08, 2.9e-06),
    3: (1.5e-06, 4.6e-08, 4.9e-08, 3.3e-06, 2.8e-08, 1.9e-06),
    12: (1.2e-06, 5.0e-08, 1.7e-08, 1.1e-06, 1.1e-08, 7.4e-07),
    13: (1.3e-06, 4.9e-08, 1.9e-08, 1.3e-06, 1.0e-08, 7.1e-07),
    15: (1.2e-06, 4.5e-08, 2.3e-08, 1.6e-06, 1.1e-08, 7.3e-07),
    16: (1.1e-06, 4.3e-08, 1.5e-08, 1.0e-06, 9.6e-09, 6.4e-07),
    17: (1.1e-06, 4.8e-08, 4.1e-08, 2.8e-06, 9.1e-09, 6.3e-07),
    19: (1.1e-06, 4.1e-08, 1.8e-08, 1.2e-06, 8.6e-09, 5.8e-07),
    20: (1.2e-06, 5.2e-08, 2.4e-08, 1.5e-06, 9.5e-09, 6.2e-07),
    28: (1.0e-06, 4.1e-08, 2.0e-08, 1.3e-06, 6.5e-09, 4.2e-07),
    29: (1.2e-06, 3.9e-08, 9.9e-09, 6.8e-07, 6.3e-09, 4.4e-07),
    32: (1.1e-06, 5.1e-08, 1.8e-08, 1.2e-06, 7.0e-09, 4.7e-07),
    33: (1.2e-06, 4.1e-08, 2.6e-08, 1.8e-06, 3.7e-08, 5.2e-07),
    42: (1.2e-06, 4.6e-08, 2.1e-08, 1.4e-06, 5.9e-09, 3.9e-07),
    43: (1.2e-06, 4.5e-08, 2.2e-08, 1.5e-06, 5.8e-09, 3.9e-07),
    63: (1.1e-06, 5.1e-08, 1.5e-08, 9.9e-07, 4.8e-09, 3.2e-07),
    64: (1.1e-06, 4.2e-08, 3.4e-08, 2.3e-06, 3.0e-08, 3.3e-07),
}

Case = collections.namedtuple("Case", "K T pairs kp instantiation chunks")


def points(K):
    if K == 10:
        return P.EXAMPLE_POINTS
    return np.random.default_rng(100 + K).uniform(-60, 60, (K, 3)).astype(np.float32)


def poses(n, seed, limit=30.0):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 6), np.float32)
    x[:, :3] = rng.uniform(-limit, limit, (n, 3))
    x[:, 5] = -2000.0
    return x


def homogeneous(pts):
    return np.concatenate([np.asarray(pts, np.float32).T, np.ones((1, len(pts)), np.float32)])


def rel_err(y, ref):
    return np.abs(np.asarray(y, np.float64) - ref).max(1) / np.abs(ref).max(1)


def start(n):
    return np.tile(P.EXAMPLE_X0, (n, 1))


def templates(x_star, pts):
    """the float64 projections of the targets, rounded to float32"""
    return P.project(x_star, pts).astype(np.float32)


def case(K):
    T = 2 * K + 6
    pairs = T * (T + 1) // 2
    kp = -(-pairs // THREADS)
    chunks = [K] if K <= CHUNK_PTS else [CHUNK_PTS] * (K // CHUNK_PTS) + ([K % CHUNK_PTS] if K % CHUNK_PTS else [])
    return Case(K, T, pairs, kp, next(i for i in GRAM_KP if i >= kp), chunks)


CASES = [case(K) for K in KS]


def lds_bytes_cascade(K, levels):
    """dynamic LDS of pose_cascade_kernel (sdm_pose_cascade_lds_bytes :352-356): regressors, points, two template tiles"""
    return (levels * 2 * K * 6 + 3 * K + 2 * THREADS * (min(K, CHUNK_PTS) + 1)) * 4


def lds_bytes_solve(K):
    """dynamic LDS of pose_solve_kernel (:400): the 2K x (2K + 6) system in double (beside 8 KiB of static reduction scratch)"""
    return 2 * K * (2 * K + 6) * 8


def gram_rows(N):
    """sdm_pose_gram_rows :376-380: rows per Gram workgroup, whole chunks, a function of N alone"""
    per = -(-N // GRAM_BLOCKS)
    return -(-per // GRAM_CHUNK) * GRAM_CHUNK


def gram_blocks(N):
    return -(-N // gram_rows(N))


# ---- float32 in the kernel's order ------------------------------------------------------------------------------------------------------
def _mat4_mul(a, b):
    c = np.empty(np.broadcast_shapes(a.shape, b.shape), np.float32)
    for i in range(4):
        for j in range(4):
            c[..., i, j] = a[..., i, 0] * b[..., 0, j] + a[..., i, 1] * b[..., 1, j] + a[..., i, 2] * b[..., 2, j] + a[..., i, 3] * b[..., 3, j]
    return c


def camera32(focal=1800.0, width=1000.0, height=1000.0, near=1.0, far=5000.0):
    """the projection matrix as sdm_pose_set_model builds it, in float32 (csrc/sdm_capi_pose.hip :58-64)"""
    f32 = np.float32
    fovy = (f32(2.0) * np.arctan2(f32(height), f32(2.0) * f32(focal))) * f32(180 / np.pi)
    rad = (fovy / f32(2.0)) * f32(np.pi) / f32(180.0)
    cotan = np.cos(rad) / np.sin(rad)
    n, fa = f32(near), f32(far)
    M = np.zeros((4, 4), np.float32)
    M[0, 0], M[1, 1] = cotan / (f32(width) / f32(height)), cotan
    M[2, 2], M[2, 3], M[3, 2] = -(n + fa) / (fa - n), (f32(-2.0) * n * fa) / (fa - n), -1.0
    return M


def _mvp32(x):
    f32, n = np.float32, x.shape[0]
    r = x[:, :3] * f32(np.pi / 180)
    c, s = np.cos(r), np.sin(r)
    one, zero = np.ones(n, f32), np.zeros(n, f32)
    mk = lambda *rows: np.stack([np.stack(r, -1) for r in rows], -2)   # noqa: E731
    T = mk((one, zero, zero, x[:, 3]), (zero, one, zero, x[:, 4]), (zero, zero, one, x[:, 5]), (zero, zero, zero, one))
    Ry = mk((c[:, 1], zero, s[:, 1], zero), (zero, one, zero, zero), (-s[:, 1], zero, c[:, 1], zero), (zero, zero, zero, one))
    Rx = mk((one, zero, zero, zero), (zero, c[:, 0], -s[:, 0], zero), (zero, s[:, 0], c[:, 0], zero), (zero, zero, zero, one))
    Rz = mk((c[:, 2], -s[:, 2], zero, zero), (s[:, 2], c[:, 2], zero, zero), (zero, zero, one, zero), (zero, zero, zero, one))
    return _mat4_mul(camera32()[None], _mat4_mul(_mat4_mul(_mat4_mul(T, Ry), Rx), Rz))           # pose_mvp :47-61


def project32(x, pts, focal=1800.0, width=1000.0, height=1000.0):
    """N x 6 float32 rows -> N x 2K float32 [u.., v..]: pose_mvp and pose_point (:47-75), operation by operation"""
    f32 = np.float32
    x = np.atleast_2d(np.asarray(x, f32))
    pts = np.asarray(pts, f32)
    mvp = _mvp32(x)
    X, Y, Z = (pts[:, k][None, :] for k in range(3))
    c0, c1, c3 = (mvp[:, r, 0:1] * X + mvp[:, r, 1:2] * Y + mvp[:, r, 2:3] * Z + mvp[:, r, 3:4] for r in (0, 1, 3))
    nx, ny = c0 / c3, c1 / c3
    hw, hh = f32(width) / f32(2.0), f32(height) / f32(2.0)
    x_ss = (nx + f32(1.0)) * hw
    y_ss = f32(height) - (ny + f32(1.0)) * hh
    out = np.concatenate([(x_ss - hw) / f32(focal), (y_ss - hh) / f32(focal)], 1)
    assert out.dtype == f32
    return out


def update32(x, tmpl, R, pts):
    """x - (project32(x) - tmpl) R with the six sums in the cascade kernel's order (:126-136): point by point, u before v"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    R = np.asarray(R, np.float32)
    K = len(pts)
    obs = project32(x, pts) - np.asarray(tmpl, np.float32)
    acc = np.zeros((x.shape[0], 6), np.float32)
    for i in range(K):
        acc = acc + obs[:, i:i + 1] * R[i][None, :] + obs[:, K + i:K + i + 1] * R[K + i][None, :]
    out = x - acc
    assert out.dtype == np.float32
    return out


def solve64(A, b, lam, regularise_last_row):
    """(R, cond) of (A^T A + Lambda) R = A^T b in float64 with the given lambda (as a Manual regulariser would set it)"""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    d = np.full(A.shape[1], float(lam))
    if not regularise_last_row:
        d[-1] = 0.0
    M = A.T @ A + np.diag(d)
    return np.linalg.solve(M, A.T @ b), np.linalg.cond(M)


def level32(xk, x_star, tmpl, pts, reg_type=1, param=2.0, regularise_last_row=True):
    """One teacher-forced level: float32 rows [project32(x_k) - t | x_k - x*], the float64 solve with the reference's float lambda
    rule, R rounded to float32, the float32 update.  Returns (R32, lambda, x_{k+1})."""
    xk, x_star = np.asarray(xk, np.float32), np.asarray(x_star, np.float32)
    A = project32(xk, pts) - np.asarray(tmpl, np.float32)
    R, lam = P.solve_level(A, xk - x_star, reg_type, param, regularise_last_row)
    R = R.astype(np.float32)
    return R, lam, update32(xk, tmpl, R, pts)


def level64(xk, x_star, tmpl, pts, reg_type=1, param=2.0, regularise_last_row=True):
    """The same level in float64 from the same x_k, as tests/test_gpu_pose.py states it.  Returns (R64, lambda, x_{k+1})."""
    obs = P.project(xk, pts) - tmpl
    R, lam = P.solve_level(obs, np.asarray(xk, np.float64) - x_star, reg_type, param, regularise_last_row)
    return R, lam, xk - obs @ R


def cascade32(x0, tmpl, Rs, pts):
    x = np.atleast_2d(np.asarray(x0, np.float32))
    for R in Rs:
        x = update32(x, tmpl, R, pts)
    return x


def cascade64(x0, tmpl, Rs, pts):
    return P.test(x0, tmpl, [np.asarray(R, np.float64) for R in Rs], pts)


def x_errors(x, x64, x_star):
    """(||x - x64|| / ||x*||, the same over the three angles)"""
    x, xs = np.asarray(x, np.float64), np.asarray(x_star, np.float64)
    return (np.linalg.norm(x - x64) / np.linalg.norm(xs), np.linalg.norm(x[:, :3] - x64[:, :3]) / np.linalg.norm(xs[:, :3]))


def x_bounds(x32, x64, x_star):
    """the project's bounds, or four times the float32 restatement's own error on this case where that is larger"""
    full, ang = x_errors(x32, x64, x_star)
    return max(X_TOL, 4.0 * full), max(ANGLE_TOL, 4.0 * ang)


def random_regressors(K, n_levels, tmpl, pts, seed, share=0.25):
    """n_levels regressors of default_rng entries, scaled so that the first update moves no parameter by more than ``share`` (degrees;
    the observed rows grow as x drifts, an update stays below one degree -- checked where they are used)"""
    obs = P.project(start(len(tmpl)), pts) - tmpl
    s = share / np.abs(obs).sum(1).max()
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-1.0, 1.0, (2 * K, 6)) * s).astype(np.float32) for _ in range(n_levels)]
