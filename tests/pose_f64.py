"""Float64 restatement of the head-pose cascade of the reference's examples/pose_estimation.cpp, written from its formulas
(test oracle of tests/test_pose_host.py and tests/test_gpu_pose.py; nothing here runs on the device).

  x = [r_x, r_y, r_z, t_x, t_y, t_z] (degrees, :41); MVP = P T R_y R_x R_z (:222, :58-98); P = perspective of :142-154 with
  fovy = 2 atan2(H, 2f) (:46); clip = MVP v, / w, viewport (:164-174), u = (x_ss - W/2)/f, v = (y_ss - H/2)/f (:232);
  features [u.., v..] - templates, b = x - x*, R = (A^T A + lambda I)^-1 A^T b with the reference's float lambda rule
  (regressors.hpp:126-148, MatrixNorm: param * (float)||A^T A||_F / N), x_{k+1} = x_k - observed R.
"""
import numpy as np

# the example's 10-point face model (:257-266), K x 3, and its landmark row (:325) with the ground truth it prints (:335)
EXAMPLE_POINTS = np.array([
    [-0.287526, -2.0203, 3.33725], [-0.11479, -17.2056, -13.5569], [-46.1668, 34.7219, -35.938], [-18.926, 31.5432, -29.9641],
    [19.2574, 31.5767, -30.229], [46.1914, 34.452, -36.1317], [-23.7552, -35.7461, -28.2573], [-0.0753515, -28.3064, -12.8984],
    [23.7138, -35.7886, -28.5949], [0.125511, -44.7427, -17.1411]], np.float32)
EXAMPLE_IBUG_IDS = ["31", "34", "37", "40", "43", "46", "49", "52", "55", "58"]
EXAMPLE_LANDMARKS = np.array([498, 504, 479, 498, 529, 553, 489, 503, 527, 503,
                              502, 513, 457, 465, 471, 471, 522, 522, 530, 536], np.float32)
EXAMPLE_GROUND_TRUTH = (11.0, -25.0, -10.0)
EXAMPLE_X0 = np.array([0, 0, 0, 0, 0, -2000], np.float32)


def example_templates(landmarks=EXAMPLE_LANDMARKS):
    """(landmarks - 500) / 1800 in float32, as :327."""
    return ((np.asarray(landmarks, np.float32) - np.float32(500.0)) / np.float32(1800.0)).reshape(1, -1)


def perspective(focal=1800.0, width=1000.0, height=1000.0, near=1.0, far=5000.0):
    fovy = 2.0 * np.arctan2(height, 2.0 * focal)
    cot = 1.0 / np.tan(fovy / 2.0)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = cot / (width / height), cot
    P[2, 2], P[2, 3], P[3, 2] = -(near + far) / (far - near), -2.0 * near * far / (far - near), -1.0
    return P


def mvp(x, P):
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    r = np.deg2rad(x[:, :3])
    c, s = np.cos(r), np.sin(r)
    M = np.zeros((n, 4, 4))
    Rx, Ry, Rz, T = (np.tile(np.eye(4), (n, 1, 1)) for _ in range(4))
    Rx[:, 1, 1], Rx[:, 1, 2], Rx[:, 2, 1], Rx[:, 2, 2] = c[:, 0], -s[:, 0], s[:, 0], c[:, 0]
    Ry[:, 0, 0], Ry[:, 0, 2], Ry[:, 2, 0], Ry[:, 2, 2] = c[:, 1], s[:, 1], -s[:, 1], c[:, 1]
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1] = c[:, 2], -s[:, 2], s[:, 2], c[:, 2]
    T[:, 0, 3], T[:, 1, 3], T[:, 2, 3] = x[:, 3], x[:, 4], x[:, 5]
    M = T @ Ry @ Rx @ Rz
    return P[None] @ M


def project(x, points=EXAMPLE_POINTS, focal=1800.0, width=1000.0, height=1000.0, near=1.0, far=5000.0):
    """N x 6 parameters -> N x 2K normalised projections [u.., v..] in float64."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    pts = np.asarray(points, np.float64)
    V = np.concatenate([pts, np.ones((pts.shape[0], 1))], 1).T                # 4 x K
    clip = mvp(x, perspective(focal, width, height, near, far)) @ V[None]     # N x 4 x K
    nx, ny = clip[:, 0] / clip[:, 3], clip[:, 1] / clip[:, 3]
    x_ss = (nx + 1.0) * width / 2.0
    y_ss = height - (ny + 1.0) * height / 2.0
    return np.concatenate([(x_ss - width / 2.0) / focal, (y_ss - height / 2.0) / focal], 1)


def reference_lambda(AtA, n, reg_type=1, param=2.0):
    """Regulariser::get_matrix's lambda (regressors.hpp:126-148) in float32 arithmetic on the float32 value of ||AtA||_F."""
    if reg_type == 0:
        return np.float32(param)
    fro = np.float32(np.sqrt(np.sum(np.asarray(AtA, np.float32).astype(np.float64) ** 2)))
    return np.float32(np.float32(param) * fro) / np.float32(n)


def solve_level(A, b, reg_type=1, param=2.0, regularise_last_row=True):
    """R = (A^T A + Lambda)^-1 A^T b in float64 (PartialPivLUSolver, regressors.hpp:199-234), float lambda; returns (R, lambda)."""
    A = np.asarray(A, np.float64)
    G = A.T @ A
    lam = reference_lambda(G, A.shape[0], reg_type, param)
    d = np.full(G.shape[0], float(lam))
    if not regularise_last_row:
        d[-1] = 0.0
    return np.linalg.solve(G + np.diag(d), A.T @ np.asarray(b, np.float64)), lam


def train(x_star, x0, templates, n_levels=3, points=EXAMPLE_POINTS, reg_type=1, param=2.0, regularise_last_row=True):
    """The whole known-template cascade in float64: returns (regressors, x after every level)."""
    x = np.asarray(x0, np.float64)
    Rs, xs = [], []
    for _ in range(n_levels):
        obs = project(x, points) - templates
        R, _ = solve_level(obs, x - x_star, reg_type, param, regularise_last_row)
        x = x - obs @ R
        Rs.append(R)
        xs.append(x)
    return Rs, xs


def test(x0, templates, Rs, points=EXAMPLE_POINTS):
    x = np.atleast_2d(np.asarray(x0, np.float64))
    for R in Rs:
        x = x - (project(x, points) - templates) @ R
    return x
