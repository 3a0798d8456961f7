// sdm_pose.hip -- 6-DOF head pose from 2D landmarks on the device: the ModelProjection cascade of the reference's
// examples/pose_estimation.cpp (a known-template SDM over three LinearRegressor<> levels, :281-283) as batched gfx950 kernels.
//
// Per parameter row x = [r_x, r_y, r_z, t_x, t_y, t_z] (angles in degrees, deg2rad :41) every kernel below builds
//     MVP = P * T(t) * R_y(r_y) * R_x(r_x) * R_z(r_z)                (model matrix :222, rotations :58-98)
// with the perspective P of :142-154 (fovy = rad2deg(2 atan2(H, 2f)) :46, aspect W/H), built once on the host (PoseCamDev), and
// projects every model point v = (X, Y, Z, 1):  clip = MVP v, divide by w, viewport x_ss = (c_x+1) W/2, y_ss = H - (c_y+1) H/2
// (:164-174), normalised u = (x_ss - W/2) / f, v = (y_ss - H/2) / f (:232).  The feature row is [u_0..u_{K-1}, v_0..v_{K-1}], no
// bias column (regressors.hpp:345-350); the known-template SDM subtracts the template (superviseddescent.hpp:195-197, 287-292) and,
// with NoNormalisation, updates x_{k+1} = x_k - observed * R_k.
//
//   pose_cascade_kernel       test / predict: one lane per row, ALL levels of a run in one launch, no feature row materialised
//                             (templates staged through LDS with coalesced loads)
//   pose_project_kernel       training: [features - templates | x - x*] as one N x (2K + 6) matrix (through an LDS tile: coalesced)
//   pose_gram_partial_kernel  upper triangle of [A|b]^T [A|b] per workgroup over a FIXED row range, products and sums in double
//   pose_gram_reduce_kernel   sums the workgroups' partials in double in block order: bit-identical for the same N
//   pose_solve_kernel         one workgroup: Regulariser::get_matrix (regressors.hpp:126-148) + LU with partial pivoting in
//                             double in LDS (PartialPivLUSolver, regressors.hpp:199-234) -> R (2K x 6)
//   pose_gather_kernel        detect -> pose hand-off: K landmark positions of every row of the landmark state, normalised by the
//                             row's own image centre and a focal length
//
// All arithmetic on the rows is float32 with -ffp-contract=off (csrc/Makefile) and the accurate sinf / cosf, in one fixed order per
// lane: a row's result does not depend on N, on the batch it is in, or on whether the levels run in one launch or one by one.
#include "sdm_kernels.h"

namespace {

constexpr int POSE_THREADS = 256;
constexpr int POSE_GRAM_CHUNK = 64;                     // rows staged in LDS per step of the Gram kernel
constexpr int POSE_GRAM_BLOCKS = 512;                   // target workgroup count of the Gram kernel (2 per CU; more only lengthens the reduce)
constexpr int POSE_MAXP = (SDM_POSE_MAX_T * (SDM_POSE_MAX_T + 1) / 2 + POSE_THREADS - 1) / POSE_THREADS;   // pairs per thread
constexpr int POSE_SOLVE_THREADS = 1024;
constexpr int POSE_CHUNK_PTS = 16;                      // model points per staged template chunk of the cascade kernel
constexpr int POSE_PROJ_ROWS = 64;                      // rows (one wave) per workgroup of the projection kernel

// c = a * b for row-major 4x4 float matrices, every entry summed k = 0..3 in order (no contraction)
__device__ __forceinline__ void mat4_mul(const float* a, const float* b, float* c)
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c[i * 4 + j] = a[i * 4 + 0] * b[0 * 4 + j] + a[i * 4 + 1] * b[1 * 4 + j] + a[i * 4 + 2] * b[2 * 4 + j] + a[i * 4 + 3] * b[3 * 4 + j];
}

// MVP of one parameter row (pose_estimation.cpp:216-222 with the projection matrix of :224-226 applied on the left)
__device__ __forceinline__ void pose_mvp(const float* x, const PoseCamDev& cam, float* mvp)
{
    const float d2r = (float)(3.14159265358979323846 / 180.0);          // deg2rad, :41
    const float rx = x[0] * d2r, ry = x[1] * d2r, rz = x[2] * d2r;
    const float cx = cosf(rx), sx = sinf(rx), cy = cosf(ry), sy = sinf(ry), cz = cosf(rz), sz = sinf(rz);
    const float T[16] = {1.f, 0.f, 0.f, x[3], 0.f, 1.f, 0.f, x[4], 0.f, 0.f, 1.f, x[5], 0.f, 0.f, 0.f, 1.f};
    const float Ry[16] = {cy, 0.f, sy, 0.f, 0.f, 1.f, 0.f, 0.f, -sy, 0.f, cy, 0.f, 0.f, 0.f, 0.f, 1.f};
    const float Rx[16] = {1.f, 0.f, 0.f, 0.f, 0.f, cx, -sx, 0.f, 0.f, sx, cx, 0.f, 0.f, 0.f, 0.f, 1.f};
    const float Rz[16] = {cz, -sz, 0.f, 0.f, sz, cz, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float a[16], b[16];
    mat4_mul(T, Ry, a);
    mat4_mul(a, Rx, b);
    mat4_mul(b, Rz, a);                  // model matrix
    mat4_mul(cam.P, a, mvp);             // projection * model
}

// normalised image coordinates of one model point (X, Y, Z, 1)
__device__ __forceinline__ void pose_point(const float* mvp, const PoseCamDev& cam, float X, float Y, float Z, float& u, float& v)
{
    const float c0 = mvp[0] * X + mvp[1] * Y + mvp[2] * Z + mvp[3];
    const float c1 = mvp[4] * X + mvp[5] * Y + mvp[6] * Z + mvp[7];
    const float c3 = mvp[12] * X + mvp[13] * Y + mvp[14] * Z + mvp[15];
    const float nx = c0 / c3, ny = c1 / c3;                              // divide by w, :158-159
    const float hw = cam.W / 2.0f, hh = cam.H / 2.0f;
    const float x_ss = (nx + 1.0f) * hw;                                 // viewport, :161-162
    const float y_ss = cam.H - (ny + 1.0f) * hh;
    u = (x_ss - hw) / cam.f;                                             // :232
    v = (y_ss - hh) / cam.f;
}

// test / predict.  LDS: the regressors of the n_levels levels (n_levels x 2K x 6), the model points (K x 3) and the templates of the
// workgroup's rows, staged through LDS with coalesced loads (one lane per row reading its own template row straight from HBM touches a
// different cache line in every lane: 2K x 64 lines per wave).  K <= POSE_CHUNK_PTS: the block's template rows -- contiguous in HBM --
// are staged once for all levels; larger K: POSE_CHUNK_PTS points at a time, per level.  The summation order over the points is the
// same either way.  HBM per row: the template (8K bytes; per level for K > POSE_CHUNK_PTS, from L2 after the first) + x in and out (48).
__global__ __launch_bounds__(POSE_THREADS) void pose_cascade_kernel(float* __restrict__ x, const float* __restrict__ tmpl,
                                                                    const float* __restrict__ R, const float* __restrict__ pts,
                                                                    PoseCamDev cam, int N, int n_levels)
{
    extern __shared__ float sm[];
    const int K = cam.K, F = 2 * K, tid = threadIdx.x;
    const int CP = K < POSE_CHUNK_PTS ? K : POSE_CHUNK_PTS, ld = CP + 1;      // (odd row stride: the lanes -- rows -- hit distinct banks)
    float* sR = sm;
    float* sP = sR + (size_t)n_levels * F * 6;
    float* sU = sP + 3 * K;
    float* sV = sU + POSE_THREADS * ld;
    for (int e = tid; e < n_levels * F * 6; e += POSE_THREADS) sR[e] = R[e];
    for (int e = tid; e < 3 * K; e += POSE_THREADS) sP[e] = pts[e];
    const long long row0 = (long long)blockIdx.x * POSE_THREADS;
    const int nrows = N - row0 < POSE_THREADS ? (int)(N - row0) : POSE_THREADS;
    const bool live = tid < nrows;
    const float* tb = tmpl + row0 * F;
    const bool resident = K <= POSE_CHUNK_PTS;
    if (resident)                                            // the block's rows: nrows x 2K contiguous floats
        for (int e = tid; e < nrows * F; e += POSE_THREADS) {
            const int r = e / F, c = e % F;
            if (c < K) sU[r * ld + c] = tb[e]; else sV[r * ld + c - K] = tb[e];
        }
    __syncthreads();
    float xr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, -1.f};         // (lanes past N compute on a harmless pose and store nothing)
    if (live)
#pragma unroll
        for (int j = 0; j < 6; ++j) xr[j] = x[(row0 + tid) * 6 + j];
    for (int l = 0; l < n_levels; ++l) {
        float mvp[16];
        pose_mvp(xr, cam, mvp);
        const float* Rl = sR + (size_t)l * F * 6;
        float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < K; c0 += CP) {
            const int cn = K - c0 < CP ? K - c0 : CP;
            if (!resident) {
                __syncthreads();
                for (int e = tid; e < nrows * cn; e += POSE_THREADS) {
                    const int r = e / cn, c = e % cn;
                    sU[r * ld + c] = tb[(size_t)r * F + c0 + c];
                    sV[r * ld + c] = tb[(size_t)r * F + K + c0 + c];
                }
                __syncthreads();
            }
            for (int c = 0; c < cn; ++c) {
                const int i = c0 + c;
                float u, v;
                pose_point(mvp, cam, sP[3 * i], sP[3 * i + 1], sP[3 * i + 2], u, v);
                const float ou = u - sU[tid * ld + c], ov = v - sV[tid * ld + c];
#pragma unroll
                for (int j = 0; j < 6; ++j) acc[j] = acc[j] + ou * Rl[i * 6 + j] + ov * Rl[(K + i) * 6 + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) xr[j] = xr[j] - acc[j];
    }
    if (live)
#pragma unroll
        for (int j = 0; j < 6; ++j) x[(row0 + tid) * 6 + j] = xr[j];
}

// training: row n of out (width W = 2K, or 2K + 6 with targets) = [u - t_u, v - t_v (, x - x*)]; tmpl / xstar may be null.
// One wave per 64 rows: the block's template rows and output rows are contiguous in HBM and go through an LDS tile [64][W | 1] with
// coalesced loads and stores; each lane projects its own row in the tile.
__global__ __launch_bounds__(POSE_PROJ_ROWS) void pose_project_kernel(const float* __restrict__ x, const float* __restrict__ xstar,
                                                                      const float* __restrict__ tmpl, const float* __restrict__ pts,
                                                                      PoseCamDev cam, int N, float* __restrict__ out, int W)
{
    extern __shared__ float tile[];
    const int K = cam.K, F = 2 * K, tid = threadIdx.x, ld = W | 1;
    const long long row0 = (long long)blockIdx.x * POSE_PROJ_ROWS;
    const int nrows = N - row0 < POSE_PROJ_ROWS ? (int)(N - row0) : POSE_PROJ_ROWS;
    if (tmpl)
        for (int e = tid; e < nrows * F; e += POSE_PROJ_ROWS) tile[(e / F) * ld + e % F] = tmpl[row0 * F + e];
    __syncthreads();
    if (tid < nrows) {
        const long long row = row0 + tid;
        float xr[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) xr[j] = x[row * 6 + j];
        float mvp[16];
        pose_mvp(xr, cam, mvp);
        float* o = tile + tid * ld;
        for (int i = 0; i < K; ++i) {
            float u, v;
            pose_point(mvp, cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], u, v);
            o[i] = tmpl ? u - o[i] : u;
            o[K + i] = tmpl ? v - o[K + i] : v;
        }
        if (xstar)
#pragma unroll
            for (int j = 0; j < 6; ++j) o[F + j] = xr[j] - xstar[row * 6 + j];      // superviseddescent.hpp:199-205
    }
    __syncthreads();
    for (int e = tid; e < nrows * W; e += POSE_PROJ_ROWS) out[row0 * W + e] = tile[(e / W) * ld + e % W];
}

// upper-triangle pair number p of a T x T matrix -> (i, j), i <= j, row-major over the triangle
__device__ __forceinline__ void pose_pair(int p, int T, int& i, int& j)
{
    int r = p, a = 0;
    while (r >= T - a) { r -= T - a; ++a; }
    i = a; j = a + r;
}

// partial[blockIdx.x][p] = sum over rows [blockIdx.x * rows, +rows) of Ab[r][i] * Ab[r][j] in double, rows in order.  The row range
// of a workgroup depends on N alone (sdm_pose_gram_rows), so the partials (and the reduce's sums) are reproducible.
// KP = pairs per thread, a compile-time bound >= ceil(npairs / 256) (no per-row branch on the pair count)
template <int KP>
__global__ __launch_bounds__(POSE_THREADS) void pose_gram_partial_kernel(const float* __restrict__ Ab, int N, int T, int rows,
                                                                         double* __restrict__ partial)
{
    __shared__ float tile[POSE_GRAM_CHUNK * SDM_POSE_MAX_T];
    const int npairs = T * (T + 1) / 2;
    unsigned off[KP];                                                    // i | j << 16 of this thread's pairs ((0, 0) past the last)
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        acc[k] = 0.0;
        off[k] = 0;
        const int p = threadIdx.x + k * POSE_THREADS;
        if (p < npairs) { int i, j; pose_pair(p, T, i, j); off[k] = (unsigned)i | ((unsigned)j << 16); }
    }
    const long long r0 = (long long)blockIdx.x * rows;
    const long long r1 = r0 + rows < N ? r0 + rows : N;
    for (long long base = r0; base < r1; base += POSE_GRAM_CHUNK) {
        const int nr = (int)(r1 - base < POSE_GRAM_CHUNK ? r1 - base : POSE_GRAM_CHUNK);
        __syncthreads();
        const float* src = Ab + base * T;
        for (int e = threadIdx.x; e < nr * T; e += POSE_THREADS) tile[e] = src[e];
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const float* tr = tile + r * T;
#pragma unroll
            for (int k = 0; k < KP; ++k) acc[k] += (double)tr[off[k] & 0xffffu] * (double)tr[off[k] >> 16];
        }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int p = threadIdx.x + k * POSE_THREADS;
        if (p < npairs) partial[(size_t)blockIdx.x * npairs + p] = acc[k];
    }
}

__global__ __launch_bounds__(POSE_THREADS) void pose_gram_reduce_kernel(const double* __restrict__ partial, int nblk, int npairs,
                                                                        double* __restrict__ G)
{
    const int p = blockIdx.x * POSE_THREADS + threadIdx.x;
    if (p >= npairs) return;
    // eight interleaved partial sums (independent loads in flight), combined in a fixed order: reproducible for the same N
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int b = 0;
    for (; b + 8 <= nblk; b += 8)
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += partial[(size_t)(b + k) * npairs + p];
    for (int k = 0; b + k < nblk; ++k) s[k] += partial[(size_t)(b + k) * npairs + p];
    G[p] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// One workgroup.  LDS: the F x T system [AtA + reg | Atb] in double (<= 128 x 134 x 8 = 137 KiB) + reduction scratch.
// Regulariser (regressors.hpp:126-148): Manual lambda = param; MatrixNorm lambda = param * (float)||AtA||_F / N, the norm over the
// float32 values of AtA as cv::norm sees them; regularise_last_row == 0 leaves the last diagonal entry alone.  Then LU with partial
// pivoting (the first largest |a_ik| of the column, as Eigen's maxCoeff): a zero pivot column is skipped like Eigen's PartialPivLU
// does, and the substitution then divides by it -- a singular system returns whatever that computes, never an error.
__global__ __launch_bounds__(POSE_SOLVE_THREADS) void pose_solve_kernel(const double* __restrict__ G, int F, int T, int reg_type,
                                                                        float param, int n_train, int regularise_last_row,
                                                                        float* __restrict__ R, float* __restrict__ lambda_out)
{
    extern __shared__ double a[];          // [F][T]
    __shared__ double red[POSE_SOLVE_THREADS];
    __shared__ int piv_s;
    __shared__ double lam_s;
    const int tid = threadIdx.x;
    for (int e = tid; e < F * T; e += POSE_SOLVE_THREADS) {
        const int i = e / T, j = e % T;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        a[e] = G[lo * T - lo * (lo - 1) / 2 + (hi - lo)];
    }
    __syncthreads();
    // ||AtA||_F^2 over the float32 values, fixed per-thread ranges + a fixed tree: reproducible
    double s = 0.0;
    for (int e = tid; e < F * F; e += POSE_SOLVE_THREADS) {
        const double g = (double)(float)a[(e / F) * T + e % F];
        s += g * g;
    }
    red[tid] = s;
    __syncthreads();
    for (int w = POSE_SOLVE_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        float lambda = param;
        if (reg_type == 1) lambda = param * (float)sqrt(red[0]) / (float)n_train;     // regressors.hpp:135
        lam_s = (double)lambda;
        if (lambda_out) lambda_out[0] = lambda;
    }
    __syncthreads();
    for (int i = tid; i < F; i += POSE_SOLVE_THREADS)
        if (regularise_last_row || i != F - 1) a[i * T + i] += lam_s;
    __syncthreads();

    for (int k = 0; k < F; ++k) {
        if (tid < 64) {                    // pivot search by wave 0: first row of the largest magnitude
            double best = -1.0;
            int bi = F;
            for (int i = k + tid; i < F; i += 64) {
                const double m = fabs(a[i * T + k]);
                if (m > best) { best = m; bi = i; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (tid == 0) piv_s = bi;
        }
        __syncthreads();
        const int p = piv_s;
        if (p != k && p < F)
            for (int j = tid; j < T; j += POSE_SOLVE_THREADS) { const double t = a[k * T + j]; a[k * T + j] = a[p * T + j]; a[p * T + j] = t; }
        __syncthreads();
        const double pv = a[k * T + k];
        if (pv != 0.0) {
            for (int i = k + 1 + tid; i < F; i += POSE_SOLVE_THREADS) a[i * T + k] = a[i * T + k] / pv;
            __syncthreads();
            const int nr = F - k - 1, nc = T - k - 1;
            for (int e = tid; e < nr * nc; e += POSE_SOLVE_THREADS) {
                const int i = k + 1 + e / nc, j = k + 1 + e % nc;
                a[i * T + j] = a[i * T + j] - a[i * T + k] * a[k * T + j];
            }
        }
        __syncthreads();
    }
    // back substitution U x = y on the M = T - F right-hand sides (y = L^-1 P Atb already sits in columns F..T-1)
    const int M = T - F;
    for (int k = F - 1; k >= 0; --k) {
        if (tid < M) a[k * T + F + tid] = a[k * T + F + tid] / a[k * T + k];
        __syncthreads();
        for (int e = tid; e < k * M; e += POSE_SOLVE_THREADS) {
            const int i = e / M, j = e % M;
            a[i * T + F + j] = a[i * T + F + j] - a[i * T + k] * a[k * T + F + j];
        }
        __syncthreads();
    }
    for (int e = tid; e < F * M; e += POSE_SOLVE_THREADS) R[e] = (float)a[(e / M) * T + F + e % M];
}

// detect -> pose: tmpl[n] = [(x_n[idx_k] - W_n/2) / f .., (y_n[idx_k] - H_n/2) / f ..] with W_n x H_n the size of row n's image
__global__ __launch_bounds__(POSE_THREADS) void pose_gather_kernel(const float* __restrict__ xl, int L, int N, const int* __restrict__ lm,
                                                                   int K, const int* __restrict__ img_idx, const int* __restrict__ img_w,
                                                                   const int* __restrict__ img_h, float f, float* __restrict__ tmpl)
{
    const long long row = (long long)blockIdx.x * POSE_THREADS + threadIdx.x;
    if (row >= N) return;
    const int im = img_idx ? img_idx[row] : (int)row;
    const float hw = (float)img_w[im] / 2.0f, hh = (float)img_h[im] / 2.0f;
    const float* xr = xl + row * 2 * L;
    float* o = tmpl + row * 2 * K;
    for (int k = 0; k < K; ++k) {
        const int i = lm[k];
        o[k] = (xr[i] - hw) / f;
        o[K + k] = (xr[L + i] - hh) / f;
    }
}

inline unsigned pose_grid(long long n) { return (unsigned)((n + POSE_THREADS - 1) / POSE_THREADS); }

}  // namespace

size_t sdm_pose_cascade_lds_bytes(int K, int n_levels)
{
    const int cp = K < POSE_CHUNK_PTS ? K : POSE_CHUNK_PTS;
    return ((size_t)n_levels * 2 * K * 6 + 3 * (size_t)K + (size_t)2 * POSE_THREADS * (cp + 1)) * sizeof(float);
}

void sdm_launch_pose_cascade(float* x, const float* tmpl, const float* R, const float* pts, const PoseCamDev& cam, int N, int n_levels,
                             hipStream_t s)
{
    // (up to 16 levels x 128 x 6 regressor floats + the staged templates: 83 KiB at K = 64)
    SDM_SET_ATTR((const void*)pose_cascade_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    hipLaunchKernelGGL(pose_cascade_kernel, dim3(pose_grid(N)), dim3(POSE_THREADS), sdm_pose_cascade_lds_bytes(cam.K, n_levels), s,
                       x, tmpl, R, pts, cam, N, n_levels);
}

void sdm_launch_pose_project(const float* x, const float* xstar, const float* tmpl, const float* pts, const PoseCamDev& cam, int N,
                             float* out, int width, hipStream_t s)
{
    const unsigned grid = (unsigned)(((long long)N + POSE_PROJ_ROWS - 1) / POSE_PROJ_ROWS);
    hipLaunchKernelGGL(pose_project_kernel, dim3(grid), dim3(POSE_PROJ_ROWS), (size_t)POSE_PROJ_ROWS * (width | 1) * sizeof(float), s,
                       x, xstar, tmpl, pts, cam, N, out, width);
}

// rows per workgroup: about POSE_GRAM_BLOCKS workgroups, whole LDS chunks, a function of N alone
int sdm_pose_gram_rows(int N)
{
    const int per = (N + POSE_GRAM_BLOCKS - 1) / POSE_GRAM_BLOCKS;
    return (per + POSE_GRAM_CHUNK - 1) / POSE_GRAM_CHUNK * POSE_GRAM_CHUNK;
}
int sdm_pose_gram_blocks(int N) { const int rows = sdm_pose_gram_rows(N); return (N + rows - 1) / rows; }

void sdm_launch_pose_gram(const float* Ab, int N, int T, double* partial, double* G, hipStream_t s)
{
    const int rows = sdm_pose_gram_rows(N), nblk = sdm_pose_gram_blocks(N), npairs = T * (T + 1) / 2;
    const int kp = (npairs + POSE_THREADS - 1) / POSE_THREADS;
    if (kp <= 2) hipLaunchKernelGGL(pose_gram_partial_kernel<2>, dim3(nblk), dim3(POSE_THREADS), 0, s, Ab, N, T, rows, partial);
    else if (kp <= 4) hipLaunchKernelGGL(pose_gram_partial_kernel<4>, dim3(nblk), dim3(POSE_THREADS), 0, s, Ab, N, T, rows, partial);
    else if (kp <= 8) hipLaunchKernelGGL(pose_gram_partial_kernel<8>, dim3(nblk), dim3(POSE_THREADS), 0, s, Ab, N, T, rows, partial);
    else if (kp <= 16) hipLaunchKernelGGL(pose_gram_partial_kernel<16>, dim3(nblk), dim3(POSE_THREADS), 0, s, Ab, N, T, rows, partial);
    else hipLaunchKernelGGL(pose_gram_partial_kernel<POSE_MAXP>, dim3(nblk), dim3(POSE_THREADS), 0, s, Ab, N, T, rows, partial);
    hipLaunchKernelGGL(pose_gram_reduce_kernel, dim3(pose_grid(npairs)), dim3(POSE_THREADS), 0, s, (const double*)partial, nblk, npairs, G);
}

void sdm_launch_pose_solve(const double* G, int F, int T, int reg_type, float param, int n_train, int regularise_last_row, float* R,
                           float* lambda_out, hipStream_t s)
{
    // (the system is up to 128 x 134 doubles = 134 KiB of dynamic LDS beside the 8 KiB reduction buffer; set per launch: per device)
    SDM_SET_ATTR((const void*)pose_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipLaunchKernelGGL(pose_solve_kernel, dim3(1), dim3(POSE_SOLVE_THREADS), (size_t)F * T * sizeof(double), s, G, F, T, reg_type, param,
                       n_train, regularise_last_row, R, lambda_out);
}

void sdm_launch_pose_gather(const float* xl, int L, int N, const int* lm, int K, const int* img_idx, const int* img_w, const int* img_h,
                            float f, float* tmpl, hipStream_t s)
{
    hipLaunchKernelGGL(pose_gather_kernel, dim3(pose_grid(N)), dim3(POSE_THREADS), 0, s, xl, L, N, lm, K, img_idx, img_w, img_h, f, tmpl);
}
