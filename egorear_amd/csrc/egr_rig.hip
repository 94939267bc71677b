// Rig self-calibration: the cameras' rotations refined from the multi-view correspondences of a clip.
//   E(dR_0..dR_{V-1}) = sum_pairs min_p sum_v w_v |P(d_v) dR_v (R_v p + t_v)|^2 + prior_weight sum_v |dR_v - I|_F^2,   P(d) = I - d d^T
// (the ray rotated by dR^T is the camera-frame point rotated by dR: the same distance), minimised over the free cameras by
// Levenberg-Marquardt on the Gauss-Newton model, the point of every pair eliminated by its 3 x 3 Schur complement.  The ray, the
// extrinsics and the normal equations are those of egr_rays.h.
//
// Three kernels, the launches are the only barrier between workgroups:
//   rig_rays_kernel        once: the trigonometry of every (pair, view) into an fp64 workspace - d[3], w - and the pairs that count
//                          (at dR = I: two weighted views and rays::factor with min_det_ratio; the others get w = 0 in every view)
//   rig_accumulate_kernel  a thread a pair at the candidate rotations: the point, then gradient (3V), Gauss-Newton matrix (3V)^2, cost,
//                          weight sum, pair and failure counts, reduced a 3 x 3 block at a time - wave shuffles (xor butterfly: every
//                          lane holds the same sum), LDS across the waves in wave order, one record a workgroup in global memory
//   rig_step_kernel        one workgroup: the records summed in block order, the candidate judged against the accepted state, the
//                          damped system of the accepted state factored (LDL^T, 12 x 12 with the held cameras as identity rows) and
//                          the next candidate written; the last launch writes the outputs instead
// No atomics and no order that depends on scheduling: the same bits every run.  fp64 arithmetic on fp32 operands.
#include "egr_rays.h"

namespace {

constexpr int RIG_THREADS = 128, RIG_WAVES = RIG_THREADS / 64;
constexpr int N3 = 3 * rays::MAX_V;                       // 12 unknowns at the most
// one record: the upper blocks of the matrix in full 12 x 12 addressing, the gradient, then four scalars
constexpr int REC_G = N3 * N3, REC_COST = REC_G + N3, REC_WSUM = REC_COST + 1, REC_COUNT = REC_WSUM + 1, REC_FAIL = REC_COUNT + 1;
constexpr int NREC = REC_FAIL + 1;                        // 160 doubles
// the solver state at the head of the workspace
constexpr int ST_ACC = 0, ST_CAND = 36, ST_G = 72, ST_H = 84, ST_E = 228, ST_EDATA = 229, ST_WSUM = 230, ST_MU = 231, ST_EDATA0 = 232,
              ST_STEPS = 233, ST_PAIRS = 234, ST_STATUS = 235, ST_SIZE = 256;
constexpr double STATUS_FIRST = 0.0, STATUS_RUNNING = 1.0, STATUS_INVALID = 2.0;
constexpr double MU0 = 1e-4, MU_DOWN = 0.1, MU_UP = 10.0, MU_MIN = 1e-12, MU_MAX = 1e12, PIVOT_TOL = 1e-10;
constexpr int RIG_MAX_ITERATIONS = 256;

inline int64_t rig_blocks(int64_t pairs) { return (pairs + RIG_THREADS - 1) / RIG_THREADS; }
inline int64_t rig_workspace_doubles(int64_t B, int64_t V, int64_t J) { return ST_SIZE + B * J * V * 4 + rig_blocks(B * J) * NREC; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Rodrigues; below 1e-4 rad the two series (tests/rig_statement.py expm)
__host__ __device__ inline void rig_exp(const double* r, double* M) {
    const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    double a, b;
    if (th2 < 1e-8) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    const double K[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double kk = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
            M[i * 3 + j] = (i == j ? 1.0 : 0.0) + a * K[i * 3 + j] + b * kk;
        }
}

// the rotation vector of a rotation whose angle stays away from pi
__host__ __device__ inline void rig_log(const double* M, double* r) {
    const double a[3] = {0.5 * (M[7] - M[5]), 0.5 * (M[2] - M[6]), 0.5 * (M[3] - M[1])};
    const double s2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], s = sqrt(s2), c = 0.5 * (M[0] + M[4] + M[8] - 1.0);
    const double k = s < 1e-6 ? 1.0 + s2 / 6.0 : atan2(s, c) / s;
    for (int i = 0; i < 3; ++i) r[i] = a[i] * k;
}

__host__ __device__ inline void mat3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// R' = dR R, t' = dR t of view v of frame b
__device__ inline void rig_extrinsics(const float* cams, const float* ctm, int ctm_per_frame, const double* dR, int b, int v, int V, double* Rp,
                                      double* tp) {
    double R[9], t[3];
    rays::extrinsics(cams + v * rays::REC, ctm, (int64_t)(ctm_per_frame ? b : 0) * V + v, R, t);
    mat3(dR + v * 9, R, Rp);
    for (int r = 0; r < 3; ++r) tp[r] = dR[v * 9 + r * 3] * t[0] + dR[v * 9 + r * 3 + 1] * t[1] + dR[v * 9 + r * 3 + 2] * t[2];
}

__global__ __launch_bounds__(RIG_THREADS) void rig_rays_kernel(const float* coords, const float* conf, const float* cams, const float* ctm,
                                                               int ctm_per_frame, int pairs, int V, int J, float sx, float sy, float thr,
                                                               float min_det_ratio, double* ws) {
    const int idx = blockIdx.x * RIG_THREADS + threadIdx.x;
    if (idx == 0) {                                        // the solver starts at the identity, nothing accepted yet
        for (int i = 0; i < ST_SIZE; ++i) ws[i] = 0.0;
        for (int v = 0; v < rays::MAX_V; ++v)
            for (int k = 0; k < 3; ++k) ws[ST_ACC + v * 9 + k * 4] = ws[ST_CAND + v * 9 + k * 4] = 1.0;
        ws[ST_MU] = MU0;
        ws[ST_STATUS] = STATUS_FIRST;
    }
    if (idx >= pairs) return;
    double* out = ws + ST_SIZE;
    const int b = idx / J, j = idx - b * J;
    rays::normal_eq n;
    int used = 0;
    for (int v = 0; v < V; ++v) {
        rays::ray ry;
        rays::make_ray(coords, conf, cams + v * rays::REC, ((int64_t)b * V + v) * J + j, (double)sx, (double)sy, thr, ry);
        for (int k = 0; k < 3; ++k) out[(int64_t)(v * 4 + k) * pairs + idx] = ry.d[k];
        out[(int64_t)(v * 4 + 3) * pairs + idx] = ry.w;
        if (ry.w == 0.0) continue;
        double R[9], t[3];
        rays::extrinsics(cams + v * rays::REC, ctm, (int64_t)(ctm_per_frame ? b : 0) * V + v, R, t);
        rays::add_ray(R, t, ry.d, ry.w, n);
        ++used;
    }
    rays::ldl f;
    if (rays::factor(n, (double)min_det_ratio, f) && used >= 2) return;
    for (int v = 0; v < V; ++v) out[(int64_t)(v * 4 + 3) * pairs + idx] = 0.0;       // the pair does not count: no view weighs
}

struct view_terms {
    double w, q[3], r[3], Bm[9], Cm[9];
};

// what view v of a pair contributes at the point p: q = R' p + t', r = P q, B = P [q]x, C = R'^T B  (zeros for a view without weight)
__device__ inline void rig_view(const double* rays_ws, const float* cams, const float* ctm, int ctm_per_frame, const double* dR, int pairs,
                                int idx, int b, int v, int V, bool ok, const double* p, view_terms& o) {
    double d[3], Rp[9], tp[3];
    for (int k = 0; k < 3; ++k) d[k] = rays_ws[(int64_t)(v * 4 + k) * pairs + idx];
    o.w = ok ? rays_ws[(int64_t)(v * 4 + 3) * pairs + idx] : 0.0;
    rig_extrinsics(cams, ctm, ctm_per_frame, dR, b, v, V, Rp, tp);
    rays::apply(Rp, tp, p, o.q);
    const double dq = d[0] * o.q[0] + d[1] * o.q[1] + d[2] * o.q[2];
    for (int k = 0; k < 3; ++k) o.r[k] = o.q[k] - d[k] * dq;
    const double Q[9] = {0.0, -o.q[2], o.q[1], o.q[2], 0.0, -o.q[0], -o.q[1], o.q[0], 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double dQ = d[0] * Q[k] + d[1] * Q[3 + k] + d[2] * Q[6 + k];
        for (int r = 0; r < 3; ++r) o.Bm[r * 3 + k] = Q[r * 3 + k] - d[r] * dQ;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) o.Cm[i * 3 + k] = Rp[i] * o.Bm[k] + Rp[3 + i] * o.Bm[3 + k] + Rp[6 + i] * o.Bm[6 + k];
}

__global__ __launch_bounds__(RIG_THREADS) void rig_accumulate_kernel(const float* cams, const float* ctm, int ctm_per_frame, int pairs, int V,
                                                                     int J, const double* ws, double* partial) {
    __shared__ double lds[RIG_WAVES][NREC];
    __shared__ double dR[rays::MAX_V * 9];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < RIG_WAVES * NREC; i += RIG_THREADS) (&lds[0][0])[i] = 0.0;
    if (tid < rays::MAX_V * 9) dR[tid] = ws[ST_CAND + tid];
    __syncthreads();
    if (ws[ST_STATUS] == STATUS_INVALID) {                 // (uniform over the grid) nothing counts: the records are zeros
        for (int i = tid; i < NREC; i += RIG_THREADS) partial[(int64_t)blockIdx.x * NREC + i] = 0.0;
        return;
    }
    const double* rays_ws = ws + ST_SIZE;
    const int idx0 = blockIdx.x * RIG_THREADS + tid;
    const bool live = idx0 < pairs;
    const int idx = live ? idx0 : 0;                       // (a thread past the end reads pair 0 and weighs nothing: it is in the shuffles)
    const int b = idx / J;

    // the point of the pair at the candidate rotations
    rays::normal_eq n;
    int used = 0;
    for (int v = 0; v < V; ++v) {
        const double w = live ? rays_ws[(int64_t)(v * 4 + 3) * pairs + idx] : 0.0;
        if (w == 0.0) continue;
        double d[3], Rp[9], tp[3];
        for (int k = 0; k < 3; ++k) d[k] = rays_ws[(int64_t)(v * 4 + k) * pairs + idx];
        rig_extrinsics(cams, ctm, ctm_per_frame, dR, b, v, V, Rp, tp);
        rays::add_ray(Rp, tp, d, w, n);
        ++used;
    }
    const bool counted = used >= 2;
    rays::ldl f;
    const bool ok = counted && rays::factor(n, 0.0, f);    // later iterates: the positivity test alone
    double p[3] = {0.0, 0.0, 0.0};
    if (ok) {
        rays::ldl_solve(f, n.rhs, p);
    } else {
        f.d1 = f.d2 = f.d3 = 1.0;
        f.l21 = f.l31 = f.l32 = 0.0;
    }

    double cost = 0.0, wsum = 0.0;
    for (int u = 0; u < V; ++u) {
        view_terms tu;
        rig_view(rays_ws, cams, ctm, ctm_per_frame, dR, pairs, idx, b, u, V, ok, p, tu);
        cost += tu.w * (tu.r[0] * tu.r[0] + tu.r[1] * tu.r[1] + tu.r[2] * tu.r[2]);
        wsum += tu.w;
        // dE/d delta_u = 2 w (q x r)
        const double g[3] = {tu.q[1] * tu.r[2] - tu.q[2] * tu.r[1], tu.q[2] * tu.r[0] - tu.q[0] * tu.r[2], tu.q[0] * tu.r[1] - tu.q[1] * tu.r[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double s = wave_sum_f64(2.0 * tu.w * g[k]);
            if (lane == 0) lds[wave][REC_G + 3 * u + k] = s;
        }
        double Y[9];                                       // A^-1 C_u, a column at a time
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double c[3] = {tu.Cm[k], tu.Cm[3 + k], tu.Cm[6 + k]};
            double y[3];
            rays::ldl_solve(f, c, y);
            for (int i = 0; i < 3; ++i) Y[i * 3 + k] = y[i];
        }
        for (int v = 0; v <= u; ++v) {                     // block (v, u) = 2 ([v == u] w_u B^T B - w_v w_u C_v^T Y_u)
            view_terms tv = tu;                            // (a copy, not a reference picked at run time: that would be scratch)
            if (v < u) rig_view(rays_ws, cams, ctm, ctm_per_frame, dR, pairs, idx, b, v, V, ok, p, tv);
            const bool diag = v == u;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (diag && k < i) continue;           // (uniform: every lane is in every shuffle)
                    double e = -tv.w * tu.w * (tv.Cm[i] * Y[k] + tv.Cm[3 + i] * Y[3 + k] + tv.Cm[6 + i] * Y[6 + k]);
                    if (diag) e += tu.w * (tu.Bm[i] * tu.Bm[k] + tu.Bm[3 + i] * tu.Bm[3 + k] + tu.Bm[6 + i] * tu.Bm[6 + k]);
                    const double s = wave_sum_f64(2.0 * e);
                    if (lane == 0) lds[wave][(3 * v + i) * N3 + 3 * u + k] = s;
                }
        }
    }
    const double s_cost = wave_sum_f64(cost), s_wsum = wave_sum_f64(wsum), s_count = wave_sum_f64(ok ? 1.0 : 0.0),
                 s_fail = wave_sum_f64(counted && !ok ? 1.0 : 0.0);
    if (lane == 0) {
        lds[wave][REC_COST] = s_cost;
        lds[wave][REC_WSUM] = s_wsum;
        lds[wave][REC_COUNT] = s_count;
        lds[wave][REC_FAIL] = s_fail;
    }
    __syncthreads();
    for (int i = tid; i < NREC; i += RIG_THREADS) {
        double s = lds[0][i];
        for (int w = 1; w < RIG_WAVES; ++w) s += lds[w][i];
        partial[(int64_t)blockIdx.x * NREC + i] = s;
    }
}

// LDL^T of the 12 x 12 system with the components that are not free as identity rows; x = -M^-1 g.  false: a pivot not above
// tol * its diagonal entry (or NaN).  One thread, every operand in LDS.
__device__ inline bool rig_solve(const double* H, const double* g, const bool* free_, double mu, double tol, double* L, double* dg, double* y,
                                 double* x) {
    for (int j = 0; j < N3; ++j) {
        if (!free_[j]) {
            dg[j] = 1.0;
            for (int i = j + 1; i < N3; ++i) L[i * N3 + j] = 0.0;
            continue;
        }
        const double hjj = H[j * N3 + j] * (1.0 + mu);
        double dj = hjj;
        for (int k = 0; k < j; ++k) dj -= L[j * N3 + k] * L[j * N3 + k] * dg[k];
        if (!(dj > tol * hjj)) return false;
        dg[j] = dj;
        for (int i = j + 1; i < N3; ++i) {
            double s = free_[i] ? H[i * N3 + j] : 0.0;
            for (int k = 0; k < j; ++k) s -= L[i * N3 + k] * L[j * N3 + k] * dg[k];
            L[i * N3 + j] = s / dj;
        }
    }
    for (int i = 0; i < N3; ++i) {
        double s = free_[i] ? -g[i] : 0.0;
        for (int k = 0; k < i; ++k) s -= L[i * N3 + k] * y[k];
        y[i] = s;
    }
    for (int i = N3 - 1; i >= 0; --i) {
        double s = y[i] / dg[i];
        for (int k = i + 1; k < N3; ++k) s -= L[k * N3 + i] * x[k];
        x[i] = s;
    }
    return true;
}

__global__ __launch_bounds__(256) void rig_step_kernel(const float* cams, const float* ctm, int ctm_per_frame, int B, int V, int fixed_mask,
                                                       double prior_weight, int nblocks, int last, const double* partial, double* ws,
                                                       float* rotation, float* matrix, float* ctm_out, float* cost0, float* cost,
                                                       int32_t* pairs_out, int32_t* steps_out, float* grad, uint8_t* valid) {
    __shared__ double rec[NREC], H[N3 * N3], g[N3], L[N3 * N3], dg[N3], y[N3], x[N3], final_dR[rays::MAX_V * 9];
    __shared__ bool free_[N3];
    const int tid = threadIdx.x;
    for (int i = tid; i < NREC; i += 256) {                // the records in block order
        double s = 0.0;
        for (int k = 0; k < nblocks; ++k) s += partial[(int64_t)k * NREC + i];
        rec[i] = s;
    }
    if (tid < N3) free_[tid] = tid / 3 < V && !((fixed_mask >> (tid / 3)) & 1);
    __syncthreads();
    if (tid == 0) {
        double status = ws[ST_STATUS];
        if (status != STATUS_INVALID) {
            const double* cand = ws + ST_CAND;
            double prior = 0.0;
            for (int v = 0; v < V; ++v)
                for (int i = 0; i < 9; ++i) {
                    const double e = cand[v * 9 + i] - (i % 4 == 0 ? 1.0 : 0.0);
                    prior += e * e;
                }
            const double e_data = rec[REC_COST], e_c = e_data + prior_weight * prior;
            const bool sound = rec[REC_FAIL] == 0.0 && rec[REC_COUNT] > 0.0 && e_c == e_c && fabs(e_c) <= 1.7e308;
            bool accept = false;
            if (status == STATUS_FIRST) {
                accept = sound;
                if (!sound) status = STATUS_INVALID;
            } else if (sound && e_c < ws[ST_E]) {
                accept = true;
            }
            if (accept) {
                // the system of the candidate: the upper blocks mirrored, the prior's gradient 2 pw (dR_32 - dR_23, ..) and exact
                // Hessian 2 pw (tr dR I - (dR + dR^T) / 2) added
                for (int i = 0; i < N3; ++i) {
                    g[i] = rec[REC_G + i];
                    for (int k = i; k < N3; ++k) H[i * N3 + k] = H[k * N3 + i] = rec[i * N3 + k];
                }
                for (int v = 0; v < V; ++v) {
                    const double* M = cand + v * 9;
                    const double trM = M[0] + M[4] + M[8], vee[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
                    for (int i = 0; i < 3; ++i) {
                        g[3 * v + i] += 2.0 * prior_weight * vee[i];
                        for (int k = 0; k < 3; ++k)
                            H[(3 * v + i) * N3 + 3 * v + k] += 2.0 * prior_weight * ((i == k ? trM : 0.0) - 0.5 * (M[i * 3 + k] + M[k * 3 + i]));
                    }
                }
                if (status == STATUS_FIRST && !rig_solve(H, g, free_, 0.0, PIVOT_TOL, L, dg, y, x)) {
                    status = STATUS_INVALID;               // the first system does not factor: the clip does not fix the rotations
                } else {
                    for (int i = 0; i < rays::MAX_V * 9; ++i) ws[ST_ACC + i] = cand[i];
                    for (int i = 0; i < N3; ++i) ws[ST_G + i] = g[i];
                    for (int i = 0; i < N3 * N3; ++i) ws[ST_H + i] = H[i];
                    ws[ST_E] = e_c;
                    ws[ST_EDATA] = e_data;
                    if (status == STATUS_FIRST) {
                        ws[ST_WSUM] = rec[REC_WSUM];
                        ws[ST_EDATA0] = e_data;
                        ws[ST_PAIRS] = rec[REC_COUNT];
                        status = STATUS_RUNNING;
                    } else {
                        ws[ST_STEPS] += 1.0;
                        ws[ST_MU] = fmax(ws[ST_MU] * MU_DOWN, MU_MIN);
                    }
                }
            } else if (status == STATUS_RUNNING) {
                ws[ST_MU] = fmin(ws[ST_MU] * MU_UP, MU_MAX);
            }
            ws[ST_STATUS] = status;
        }
        if (status == STATUS_RUNNING && !last) {           // the next candidate, from the stored system of the accepted rotations
            for (int i = 0; i < N3; ++i) g[i] = ws[ST_G + i];
            for (int i = 0; i < N3 * N3; ++i) H[i] = ws[ST_H + i];
            const bool solved = rig_solve(H, g, free_, ws[ST_MU], 0.0, L, dg, y, x);
            for (int v = 0; v < rays::MAX_V; ++v) {
                double delta[3] = {0.0, 0.0, 0.0}, E[9], M[9];
                bool finite = solved;
                for (int k = 0; k < 3; ++k) finite = finite && fabs(x[3 * v + k]) <= 1.7e308;
                if (finite && free_[3 * v])
                    for (int k = 0; k < 3; ++k) delta[k] = x[3 * v + k];
                rig_exp(delta, E);
                mat3(E, ws + ST_ACC + v * 9, M);
                for (int i = 0; i < 9; ++i) ws[ST_CAND + v * 9 + i] = M[i];
            }
        }
        if (last) {
            const bool good = status == STATUS_RUNNING;
            double gmax = 0.0;
            for (int i = 0; i < N3; ++i)
                if (good && free_[i]) gmax = fmax(gmax, fabs(ws[ST_G + i]));
            for (int v = 0; v < rays::MAX_V; ++v)
                for (int i = 0; i < 9; ++i) final_dR[v * 9 + i] = good ? ws[ST_ACC + v * 9 + i] : (i % 4 == 0 ? 1.0 : 0.0);
            for (int v = 0; v < V; ++v) {
                double r[3];
                rig_log(final_dR + v * 9, r);
                for (int k = 0; k < 3; ++k) rotation[v * 3 + k] = good ? (float)r[k] : 0.f;
                for (int i = 0; i < 9; ++i) matrix[v * 9 + i] = (float)final_dR[v * 9 + i];
                // ctm_out composes the fp32 matrices, so that it is apply_rig_correction(matrix, ..) bit for bit: fp32 times fp32 is
                // exact in fp64 and the three products are added in index order
                for (int i = 0; i < 9; ++i) final_dR[v * 9 + i] = (double)matrix[v * 9 + i];
            }
            const double wsum = good ? ws[ST_WSUM] : 1.0;
            *cost0 = good ? (float)(ws[ST_EDATA0] / wsum) : 0.f;
            *cost = good ? (float)(ws[ST_EDATA] / wsum) : 0.f;
            *pairs_out = good ? (int32_t)ws[ST_PAIRS] : 0;
            *steps_out = good ? (int32_t)ws[ST_STEPS] : 0;
            *grad = (float)gmax;
            *valid = good ? 1 : 0;
        }
    }
    if (!last) return;
    __syncthreads();
    // [dR 0; 0 1] M of every (frame, view), in the decoders' convention: translations in m, the syn rig from the record's flip and offset
    for (int i = tid; i < B * V; i += 256) {
        const int b = i / V, v = i - b * V;
        double M[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
        if (ctm) {
            const float* m = ctm + ((int64_t)(ctm_per_frame ? b : 0) * V + v) * 16;
            for (int k = 0; k < 16; ++k) M[k] = (double)m[k];
        } else {
            const float* cam = cams + v * rays::REC;
            const double fl = cam[rays::FLIP] != 0.f ? -1.0 : 1.0;
            M[0] = M[5] = fl;
            M[10] = 1.0;
            for (int r = 0; r < 3; ++r) M[r * 4 + 3] = (double)(float)((double)cam[rays::OFF + r] * 0.01);   // (fp32, as a caller would pass it)
        }
        const double* D = final_dR + v * 9;
        float* o = ctm_out + (int64_t)i * 16;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) o[r * 4 + c] = (float)(D[r * 3] * M[c] + D[r * 3 + 1] * M[4 + c] + D[r * 3 + 2] * M[8 + c]);
        for (int c = 0; c < 4; ++c) o[12 + c] = (float)M[12 + c];
    }
}

inline bool rig_shape_ok(int32_t B, int32_t V, int32_t J, float sx, float sy, float thr, float min_det_ratio, int32_t fixed_mask,
                         float prior_weight, int32_t iterations) {
    return rays::shape_ok(B, V, J, sx, sy, min_det_ratio) && thr == thr && (int64_t)B * J < (1 << 28) && fixed_mask >= 0 &&
           fixed_mask < (1 << V) && prior_weight >= 0.f && prior_weight <= 3.0e38f && iterations >= 1 && iterations <= RIG_MAX_ITERATIONS;
}

}  // namespace

extern "C" int64_t egr_rig_refine_workspace_bytes(int32_t B, int32_t V, int32_t J) {
    if (B < 1 || J < 1 || V < 2 || V > rays::MAX_V || (int64_t)B * J >= (1 << 28)) return 0;
    return rig_workspace_doubles(B, V, J) * (int64_t)sizeof(double);
}

extern "C" int egr_rig_refine_f32(const float* coords, const float* conf, const float* cams, const float* ctm, int32_t ctm_per_frame, int32_t B,
                                  int32_t V, int32_t J, float sx, float sy, float threshold, float min_det_ratio, int32_t fixed_mask,
                                  float prior_weight, int32_t iterations, double* workspace, int64_t workspace_bytes, float* rotation,
                                  float* matrix, float* ctm_out, float* cost0, float* cost, int32_t* pairs, int32_t* steps, float* grad,
                                  uint8_t* valid, void* stream) {
    if (!coords || !conf || !cams || !workspace || !rotation || !matrix || !ctm_out || !cost0 || !cost || !pairs || !steps || !grad || !valid)
        return EGR_ENULL;
    if (!rig_shape_ok(B, V, J, sx, sy, threshold, min_det_ratio, fixed_mask, prior_weight, iterations)) return EGR_EINVAL;
    if (workspace_bytes < egr_rig_refine_workspace_bytes(B, V, J)) return EGR_EWORKSPACE;
    const int n = B * J, blocks = (int)rig_blocks(n);
    const int per_frame = ctm && ctm_per_frame ? 1 : 0;
    double* partial = workspace + ST_SIZE + (int64_t)n * V * 4;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rig_rays_kernel, dim3((unsigned)blocks), dim3(RIG_THREADS), 0, s, coords, conf, cams, ctm, per_frame, n, V, J, sx, sy,
                       threshold, min_det_ratio, workspace);
    // the start is evaluated, then every iteration judges the last evaluation, solves and evaluates its candidate; the last step
    // launch judges the last candidate and writes the outputs
    for (int it = 0; it <= iterations; ++it) {
        hipLaunchKernelGGL(rig_accumulate_kernel, dim3((unsigned)blocks), dim3(RIG_THREADS), 0, s, cams, ctm, per_frame, n, V, J,
                           (const double*)workspace, partial);
        hipLaunchKernelGGL(rig_step_kernel, dim3(1), dim3(256), 0, s, cams, ctm, per_frame, B, V, fixed_mask, (double)prior_weight, blocks,
                           it == iterations ? 1 : 0, (const double*)partial, workspace, rotation, matrix, ctm_out, cost0, cost, pairs, steps,
                           grad, valid);
    }
    return egr_launch_status();
}
