// Temporal trajectory smoothing of 3-D joints over a clip: forward (plain and Huber-reweighted) and backward.
// A track is one joint of one clip, T frames of observations z_t (cm) with base weights w_t >= 0.  Its smoothed positions solve
//   A x = W z,   A = W + lv D1^T D1 + la D2^T D2     (D1, D2: first and second differences along t)
// - symmetric, positive definite and pentadiagonal; the three coordinates share A.  With huber = delta > 0 the solve is repeated
// K = reweights more times with the weights w_t min(1, delta / |x_t - z_t|) of the previous solution (IRLS, a majorise-minimise step).
//
// One lane owns one track, the tracks of a clip in adjacent lanes: lane (n, j) reads pose[n, t, j, :], so a wave's reads at one t are
// contiguous.  A banded LDL^T along t in fp64 on the fp32 operands: the forward sweep carries d_{t-1}, d_{t-2} and the two
// sub-diagonals in registers (one fp64 division per step: the reciprocal of the pivot) and writes e_t = L[t+1][t], f_t = L[t+2][t]
// and q_t = y_t / d_t of every right-hand side to an fp64 workspace laid out (slot, t, track) - a wave's accesses at one t coalesce;
// the backward sweep substitutes x_t = q_t - e_t x_{t+1} - f_t x_{t+2}.  (1 / d_t itself is not stored: with q scaled in the forward
// sweep nothing reads it again.)  The reweighted solves read the previous x_t from the q slots they are about to overwrite, and the
// last backward sweep writes the outputs and sums the energy: every solve runs inside the one launch.  No atomics, no LDS, no
// cross-lane traffic, no exit that depends on data other than the solvable flag, a fixed order everywhere: a track's bits depend on
// its own operands only.  The kernel is bound by the latency of the dependent fp64 chain of length T (times 2 (K + 1) sweeps); the
// operands of the next chunk of frames are fetched before this chunk's steps are computed, so that the chain waits for memory once a
// chunk at the most.
#include <math.h>

#include "egr_common.h"
#include "egr_trajectory_band.h"      // trj_band: row t of the penalty

namespace {

constexpr int TRJ_MAX_T = 4096, TRJ_MAX_REWEIGHTS = 16;
constexpr int TRJ_FWD_SLOTS = 5, TRJ_BWD_SLOTS = 8;      // e, f and the q of 3 / 6 right-hand sides

struct trj_args {
    const float* pose;
    const float* weight;     // nullable: 1
    const uint8_t* obs;      // nullable: every frame
    int T, J;
    int64_t tracks;
    double lv, la, delta;
    int reweights, max_gap;
};

struct trj_frame {
    double z[3], w;          // w = 0 and z = 0 for a frame that is not observed: what was planted there is selected away, not multiplied
};

__host__ __device__ inline bool trj_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// What one frame's loads return, before any arithmetic: a chunk of them is in flight together.
struct trj_raw {
    float x, y, z, w;
    uint8_t on;
};

// (No branch on the optional operands: a branch around a load makes the compiler wait for every load in flight where the paths join,
// which puts a memory latency into every step.  Without a weight or a mask the load goes to the frame's pose - an address that is
// valid - and its value is selected away.)
__host__ __device__ inline void trj_fetch(const trj_args& p, int64_t at, trj_raw& r) {
    const float* xyz = p.pose + at * 3;
    const float w = *(p.weight ? p.weight + at : xyz);
    const uint8_t on = *(p.obs ? p.obs + at : (const uint8_t*)xyz);
    r.w = p.weight ? w : 1.0f;
    r.on = p.obs ? on : (uint8_t)1;
    r.x = xyz[0];
    r.y = xyz[1];
    r.z = xyz[2];
}

__host__ __device__ inline void trj_decode(const trj_raw& r, trj_frame& o) {
    const bool on = r.on != 0 && trj_finite(r.w) && r.w > 0.0f && trj_finite(r.x) && trj_finite(r.y) && trj_finite(r.z);
    o.w = on ? (double)r.w : 0.0;
    o.z[0] = on ? (double)r.x : 0.0;
    o.z[1] = on ? (double)r.y : 0.0;
    o.z[2] = on ? (double)r.z : 0.0;
}

// The elimination's carried state for R right-hand sides.
template <int R>
struct trj_chain {
    double d1 = 0.0, d2 = 0.0, e1 = 0.0, f1 = 0.0, f2 = 0.0, y1[R], y2[R];
    __host__ __device__ inline trj_chain() {
        for (int r = 0; r < R; ++r) y1[r] = y2[r] = 0.0;
    }
    // pivot t: diag = A[t][t], b, c as trj_band, rhs[R] -> e, f, q[R]
    __host__ __device__ inline void step(double diag, double b, double c, const double* rhs, double& e, double& f, double* q) {
        const double d = diag - e1 * e1 * d1 - f2 * f2 * d2;
        const double dinv = 1.0 / d;
        e = (b - f1 * d1 * e1) * dinv;
        f = c * dinv;
        for (int r = 0; r < R; ++r) {
            const double y = rhs[r] - e1 * y1[r] - f2 * y2[r];
            // y / d from the one reciprocal, corrected by a fused residual step: where the quotient is representable (a frame that
            // nothing couples to its neighbours: x = w z / w) it comes out exactly.  q is off the chain: only y is carried.
            const double q0 = y * dinv;
            q[r] = fma(fma(-d, q0, y), dinv, q0);
            y2[r] = y1[r];
            y1[r] = y;
        }
        d2 = d1;
        d1 = d;
        f2 = f1;
        f1 = f;
        e1 = e;
    }
};

__host__ __device__ inline int trj_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int trj_max(int a, int b) { return a > b ? a : b; }

// (eight frames' loads in flight together: the count does not wait for memory once a frame)
__host__ __device__ inline bool trj_solvable(const trj_args& p, int64_t base) {
    int seen = 0;
    for (int t0 = 0; t0 < p.T; t0 += 8) {
        trj_raw r[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) trj_fetch(p, base + (int64_t)trj_min(t0 + i, p.T - 1) * p.J, r[i]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            trj_frame o;
            trj_decode(r[i], o);
            seen += (t0 + i < p.T && o.w > 0.0) ? 1 : 0;
        }
    }
    return p.lv > 0.0 ? seen >= 1 : (p.T >= 3 ? seen >= 2 : seen == p.T);
}

__host__ __device__ inline double trj_dist(const double* x, const double* z) {
    const double a = x[0] - z[0], b = x[1] - z[1], c = x[2] - z[2];
    return sqrt(a * a + b * b + c * c);
}

constexpr int TRJ_FAR = 1 << 30;
// Steps whose operands are in flight together.  A sweep works on chunks of CH frames: the loads of the next chunk are issued, then
// the CH dependent steps of this one are computed, so that the chain waits for memory once a chunk at the most (measured with the
// operands of one step fetched one step ahead: 0.89 us a step, the latency of a load; DESIGN.md 5s has the figures of both).  The
// chunk loops are unrolled: the buffers are registers.
constexpr int TRJ_CH = 4, TRJ_CH_BWD = 4;

__host__ __device__ inline void trj_forward_one(const trj_args& p, int64_t k, double* ws, float* pose_out, uint8_t* valid, float* residual,
                                                float* weight_out, float* energy) {
    constexpr int CH = TRJ_CH;
    const int T = p.T, J = p.J;
    const int64_t n = k / J, j = k - n * J;
    const int64_t base = n * T * J + j;              // the track's frame t is element base + t * J
    const int64_t plane = (int64_t)T * p.tracks;     // one workspace slot
    if (!trj_solvable(p, base)) {
        for (int t = 0; t < T; ++t) {
            const int64_t at = base + (int64_t)t * J;
            pose_out[at * 3] = pose_out[at * 3 + 1] = pose_out[at * 3 + 2] = 0.0f;
            valid[at] = 0;
            residual[at] = weight_out[at] = 0.0f;
        }
        energy[k] = 0.0f;
        return;
    }
    double* const E = ws + k;                        // slot s of frame t: E[s * plane + t * tracks]
    for (int it = 0; it <= p.reweights; ++it) {
        const bool first = it == 0, last = it == p.reweights;
        // ---- forward sweep: factor and reduce the three right-hand sides
        {
            trj_chain<3> ch;
            trj_raw cur[CH], nxt[CH];
            double xp[CH][3], xn[CH][3];             // the previous solve's x_t, read from the q slots before they are overwritten
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int tt = trj_min(i, T - 1);
                trj_fetch(p, base + (int64_t)tt * J, cur[i]);
                for (int c = 0; c < 3; ++c) xp[i][c] = E[(2 + c) * plane + (int64_t)tt * p.tracks];      // (not used by the first sweep)
            }
            int since = TRJ_FAR;
            for (int t0 = 0; t0 < T; t0 += CH) {
#pragma unroll
                for (int i = 0; i < CH; ++i) {       // (rows ahead of every row this chunk writes; past the end the last row, unused)
                    const int tt = trj_min(t0 + CH + i, T - 1);
                    trj_fetch(p, base + (int64_t)tt * J, nxt[i]);
                    for (int c = 0; c < 3; ++c) xn[i][c] = E[(2 + c) * plane + (int64_t)tt * p.tracks];
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int t = t0 + i;
                    if (t < T) {
                        trj_frame o;
                        trj_decode(cur[i], o);
                        double w = o.w;
                        if (!first && w > 0.0) {
                            const double r = trj_dist(xp[i], o.z);
                            w = r > p.delta ? w * (p.delta / r) : w;
                        }
                        double a, b, c, e, f, q[3];
                        trj_band(t, T, p.lv, p.la, a, b, c);
                        const double rhs[3] = {w * o.z[0], w * o.z[1], w * o.z[2]};
                        ch.step(a + w, b, c, rhs, e, f, q);
                        const int64_t row = (int64_t)t * p.tracks;
                        E[row] = e;
                        E[plane + row] = f;
                        for (int r = 0; r < 3; ++r) E[(2 + r) * plane + row] = q[r];
                        if (last) {
                            const int64_t at = base + (int64_t)t * J;
                            since = o.w > 0.0 ? 0 : (since < TRJ_FAR ? since + 1 : TRJ_FAR);
                            weight_out[at] = (float)w;
                            valid[at] = since <= p.max_gap ? 1 : 0;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    cur[i] = nxt[i];
                    for (int c = 0; c < 3; ++c) xp[i][c] = xn[i][c];
                }
            }
        }
        // ---- backward sweep: substitute; the last one writes the outputs and sums the energy
        double x1[3] = {0.0, 0.0, 0.0}, x2[3] = {0.0, 0.0, 0.0};
        double e_data = 0.0, e_vel = 0.0, e_acc = 0.0;
        int until = TRJ_FAR;
        double ce[CH], cf[CH], cq[CH][3], ne[CH], nf[CH], nq[CH][3];
        trj_raw cur[CH], nxt[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int tt = trj_max(T - 1 - i, 0);
            const int64_t row = (int64_t)tt * p.tracks;
            ce[i] = E[row];
            cf[i] = E[plane + row];
            for (int c = 0; c < 3; ++c) cq[i][c] = E[(2 + c) * plane + row];
            trj_fetch(p, base + (int64_t)tt * J, cur[i]);        // (used by the last sweep only)
        }
        for (int t1 = T - 1; t1 >= 0; t1 -= CH) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {           // (rows below every row this chunk writes; past the start row 0, unused)
                const int tt = trj_max(t1 - CH - i, 0);
                const int64_t row = (int64_t)tt * p.tracks;
                ne[i] = E[row];
                nf[i] = E[plane + row];
                for (int c = 0; c < 3; ++c) nq[i][c] = E[(2 + c) * plane + row];
                trj_fetch(p, base + (int64_t)tt * J, nxt[i]);
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int t = t1 - i;
                if (t >= 0) {
                    double x[3];
                    for (int c = 0; c < 3; ++c) x[c] = cq[i][c] - ce[i] * x1[c] - cf[i] * x2[c];
                    if (!last) {
                        for (int c = 0; c < 3; ++c) E[(2 + c) * plane + (int64_t)t * p.tracks] = x[c];
                    } else {
                        trj_frame o;
                        trj_decode(cur[i], o);
                        const int64_t at = base + (int64_t)t * J;
                        for (int c = 0; c < 3; ++c) pose_out[at * 3 + c] = (float)x[c];
                        double r = 0.0;
                        if (o.w > 0.0) {
                            r = trj_dist(x, o.z);
                            e_data += o.w * (p.delta > 0.0 && r > p.delta ? 2.0 * p.delta * r - p.delta * p.delta : r * r);
                        }
                        residual[at] = (float)r;
                        if (t < T - 1) {
                            const double v0 = x1[0] - x[0], v1 = x1[1] - x[1], v2 = x1[2] - x[2];
                            e_vel += v0 * v0 + v1 * v1 + v2 * v2;
                        }
                        if (t < T - 2) {
                            const double a0 = x2[0] - 2.0 * x1[0] + x[0], a1 = x2[1] - 2.0 * x1[1] + x[1], a2 = x2[2] - 2.0 * x1[2] + x[2];
                            e_acc += a0 * a0 + a1 * a1 + a2 * a2;
                        }
                        until = o.w > 0.0 ? 0 : (until < TRJ_FAR ? until + 1 : TRJ_FAR);
                        if (until <= p.max_gap) valid[at] = 1;       // (the forward sweep wrote the flag of the frames before t)
                    }
                    for (int c = 0; c < 3; ++c) {
                        x2[c] = x1[c];
                        x1[c] = x[c];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                ce[i] = ne[i];
                cf[i] = nf[i];
                for (int c = 0; c < 3; ++c) cq[i][c] = nq[i][c];
                cur[i] = nxt[i];
            }
        }
        if (last) energy[k] = (float)(e_data + p.lv * e_vel + p.la * e_acc);
    }
}

// The plain form's backward: with u = A^-1 g_x (the same factorisation, three more right-hand sides),
//   g_z[t] = w_t u_t,   g_weight[t] = [observed_t] u_t . (z_t - x_t).
__host__ __device__ inline void trj_backward_one(const trj_args& p, int64_t k, const float* g_x, double* ws, float* g_pose, float* g_weight) {
    constexpr int CH = TRJ_CH_BWD;
    const int T = p.T, J = p.J;
    const int64_t n = k / J, j = k - n * J;
    const int64_t base = n * T * J + j;
    const int64_t plane = (int64_t)T * p.tracks;
    if (!trj_solvable(p, base)) {
        for (int t = 0; t < T; ++t) {
            const int64_t at = base + (int64_t)t * J;
            g_pose[at * 3] = g_pose[at * 3 + 1] = g_pose[at * 3 + 2] = 0.0f;
            if (g_weight) g_weight[at] = 0.0f;
        }
        return;
    }
    double* const E = ws + k;
    trj_raw cur[CH], nxt[CH];
    {
        trj_chain<6> ch;
        float gc[CH][3], gn[CH][3];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int64_t at = base + (int64_t)trj_min(i, T - 1) * J;
            trj_fetch(p, at, cur[i]);
            for (int c = 0; c < 3; ++c) gc[i][c] = g_x[at * 3 + c];
        }
        for (int t0 = 0; t0 < T; t0 += CH) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int64_t at = base + (int64_t)trj_min(t0 + CH + i, T - 1) * J;
                trj_fetch(p, at, nxt[i]);
                for (int c = 0; c < 3; ++c) gn[i][c] = g_x[at * 3 + c];
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int t = t0 + i;
                if (t < T) {
                    trj_frame o;
                    trj_decode(cur[i], o);
                    double a, b, c, e, f, q[6];
                    trj_band(t, T, p.lv, p.la, a, b, c);
                    const double rhs[6] = {o.w * o.z[0], o.w * o.z[1], o.w * o.z[2], (double)gc[i][0], (double)gc[i][1], (double)gc[i][2]};
                    ch.step(a + o.w, b, c, rhs, e, f, q);
                    const int64_t row = (int64_t)t * p.tracks;
                    E[row] = e;
                    E[plane + row] = f;
                    for (int r = 0; r < 6; ++r) E[(2 + r) * plane + row] = q[r];
                }
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                cur[i] = nxt[i];
                for (int c = 0; c < 3; ++c) gc[i][c] = gn[i][c];
            }
        }
    }
    double x1[6], x2[6];
    for (int r = 0; r < 6; ++r) x1[r] = x2[r] = 0.0;
    double ce[CH], cf[CH], cq[CH][6], ne[CH], nf[CH], nq[CH][6];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int tt = trj_max(T - 1 - i, 0);
        const int64_t row = (int64_t)tt * p.tracks;
        ce[i] = E[row];
        cf[i] = E[plane + row];
        for (int r = 0; r < 6; ++r) cq[i][r] = E[(2 + r) * plane + row];
        trj_fetch(p, base + (int64_t)tt * J, cur[i]);
    }
    for (int t1 = T - 1; t1 >= 0; t1 -= CH) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int tt = trj_max(t1 - CH - i, 0);
            const int64_t row = (int64_t)tt * p.tracks;
            ne[i] = E[row];
            nf[i] = E[plane + row];
            for (int r = 0; r < 6; ++r) nq[i][r] = E[(2 + r) * plane + row];
            trj_fetch(p, base + (int64_t)tt * J, nxt[i]);
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int t = t1 - i;
            if (t >= 0) {
                trj_frame o;
                trj_decode(cur[i], o);
                double x[6];
                for (int r = 0; r < 6; ++r) x[r] = cq[i][r] - ce[i] * x1[r] - cf[i] * x2[r];
                const int64_t at = base + (int64_t)t * J;
                for (int c = 0; c < 3; ++c) g_pose[at * 3 + c] = (float)(o.w * x[3 + c]);
                if (g_weight) {
                    const double gw = x[3] * (o.z[0] - x[0]) + x[4] * (o.z[1] - x[1]) + x[5] * (o.z[2] - x[2]);
                    g_weight[at] = o.w > 0.0 ? (float)gw : 0.0f;
                }
                for (int r = 0; r < 6; ++r) {
                    x2[r] = x1[r];
                    x1[r] = x[r];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            ce[i] = ne[i];
            cf[i] = nf[i];
            for (int r = 0; r < 6; ++r) cq[i][r] = nq[i][r];
            cur[i] = nxt[i];
        }
    }
}

__global__ __launch_bounds__(64) void trajectory_smooth_kernel(trj_args p, double* ws, float* pose_out, uint8_t* valid, float* residual,
                                                               float* weight_out, float* energy) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= p.tracks) return;
    trj_forward_one(p, k, ws, pose_out, valid, residual, weight_out, energy);
}

__global__ __launch_bounds__(64) void trajectory_smooth_bwd_kernel(trj_args p, const float* g_x, double* ws, float* g_pose, float* g_weight) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= p.tracks) return;
    trj_backward_one(p, k, g_x, ws, g_pose, g_weight);
}

inline bool trj_number(float v) { return v >= 0.0f && v <= 3.402823466e38f; }     // non-negative and finite

inline bool trj_shape_ok(int32_t N, int32_t T, int32_t J, float lv, float la) {
    if (N < 1 || J < 1 || T < 1 || T > TRJ_MAX_T) return false;
    if ((int64_t)N * T * J >= ((int64_t)1 << 31)) return false;
    return trj_number(lv) && trj_number(la) && (lv > 0.0f || la > 0.0f);
}

inline trj_args trj_pack(const float* pose, const float* weight, const uint8_t* obs, int32_t N, int32_t T, int32_t J, float lv, float la,
                         float huber, int32_t reweights, int32_t max_gap) {
    trj_args p;
    p.pose = pose;
    p.weight = weight;
    p.obs = obs;
    p.T = T;
    p.J = J;
    p.tracks = (int64_t)N * J;
    p.lv = (double)lv;
    p.la = (double)la;
    p.delta = (double)huber;
    p.reweights = reweights;
    p.max_gap = max_gap;
    return p;
}

}  // namespace

extern "C" int egr_trajectory_smooth_f32(const float* pose, const float* weight, const uint8_t* obs, int32_t N, int32_t T, int32_t J,
                                         float vel_weight, float accel_weight, float huber, int32_t reweights, int32_t max_gap,
                                         double* workspace, float* pose_out, uint8_t* valid, float* residual, float* weight_out, float* energy,
                                         void* stream) {
    if (!pose || !workspace || !pose_out || !valid || !residual || !weight_out || !energy) return EGR_ENULL;
    if (!trj_shape_ok(N, T, J, vel_weight, accel_weight)) return EGR_EINVAL;
    if (!trj_number(huber) || reweights < 0 || reweights > TRJ_MAX_REWEIGHTS || (reweights > 0) != (huber > 0.0f) || max_gap < 0)
        return EGR_EINVAL;
    const trj_args p = trj_pack(pose, weight, obs, N, T, J, vel_weight, accel_weight, huber, reweights, max_gap);
    hipLaunchKernelGGL(trajectory_smooth_kernel, dim3((unsigned)((p.tracks + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p, workspace,
                       pose_out, valid, residual, weight_out, energy);
    return egr_launch_status();
}

extern "C" int egr_trajectory_smooth_bwd_f32(const float* pose, const float* weight, const uint8_t* obs, const float* g_pose_out, int32_t N,
                                             int32_t T, int32_t J, float vel_weight, float accel_weight, double* workspace, float* g_pose,
                                             float* g_weight, void* stream) {
    if (!pose || !g_pose_out || !workspace || !g_pose) return EGR_ENULL;
    if (!trj_shape_ok(N, T, J, vel_weight, accel_weight)) return EGR_EINVAL;
    const trj_args p = trj_pack(pose, weight, obs, N, T, J, vel_weight, accel_weight, 0.0f, 0, 0);
    hipLaunchKernelGGL(trajectory_smooth_bwd_kernel, dim3((unsigned)((p.tracks + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p, g_pose_out,
                       workspace, g_pose, g_weight);
    return egr_launch_status();
}

// ---- the causal fixed-lag filter of a stream of frames ---------------------------------------------------------------
// The forward elimination above is a causal recursion: for the prefix problem over the frames 0..t only the last two rows of A carry
// boundary coefficients (trj_band(s, T) does not depend on T for s <= T - 3), so row t - 2 is final the moment frame t arrives.  A
// stream's state is the chain after its final rows, the two frames whose rows are not final yet, and a ring of the last `lag` final
// rows; the arrival of frame t commits row t - 2, takes the two provisional steps of the prefix's boundary rows on a copy of the chain
// and substitutes back `lag` rows: frame t - lag of the plain solution over 0..t.  With gate = delta > 0 the arriving observation is
// first weighed against the prediction p_t the earlier frames make for it - the last row's q of the same prefix with w_t = 0, one
// more elimination step: u_t = w_t min(1, delta / |z_t - p_t|), fixed from then on.
//
// One lane per track, the tracks of a stream in adjacent lanes.  The state is fp64, laid out (slot, track) - a wave's accesses at one
// slot coalesce:
//   0..10   the chain: d1, d2, e1, f1, f2, y1[3], y2[3]                 (trj_chain<3> after the last final row)
//   11..15  the older pending frame (t - 1 once t has arrived): u, z[3], frames since the last observed one
//   16..20  the newer pending frame (t): the same
//   21      frames seen                      22   observed frames seen, saturating at 2
//   23 + 10 r ..   row s of the ring, r = s mod lag: e, f, q[3], z[3], u, frames since the last observed one
// All zeros is the empty stream.  A reset starts slots 0..22 from zero and leaves the ring as it is: a substitution reaches only rows
// committed since, so the earlier stream's rows are never read (and a reset tensor need not be all zeros).  The band needs min(t, 2) and the distance to the prefix's end only, so no coefficient depends on a
// stream's length; slot 21 counts exactly up to 2^53 frames.  The C frames of a call run the same per-frame code one after another.
namespace {

constexpr int TRF_MAX_LAG = 64, TRF_HEAD = 23, TRF_ROW = 10;

struct trf_pend {
    double u, z[3], since;
};

struct trf_state {
    trj_chain<3> ch;
    trf_pend a, b;           // frames n - 2 and n - 1
    int64_t n;
    int seen;
};

struct trf_args {
    double lv, la, gate;
    int lag, max_gap;
    int64_t tracks;
};

__device__ inline void trf_load(const double* S, int64_t tr, bool clear, trf_state& st) {
    double v[TRF_HEAD];
#pragma unroll
    for (int i = 0; i < TRF_HEAD; ++i) v[i] = S[i * tr];
#pragma unroll
    for (int i = 0; i < TRF_HEAD; ++i) v[i] = clear ? 0.0 : v[i];
    st.ch.d1 = v[0], st.ch.d2 = v[1], st.ch.e1 = v[2], st.ch.f1 = v[3], st.ch.f2 = v[4];
    for (int c = 0; c < 3; ++c) st.ch.y1[c] = v[5 + c], st.ch.y2[c] = v[8 + c], st.a.z[c] = v[12 + c], st.b.z[c] = v[17 + c];
    st.a.u = v[11], st.a.since = v[15], st.b.u = v[16], st.b.since = v[20];
    st.n = (int64_t)v[21];
    st.seen = (int)v[22];
}

__device__ inline void trf_store(double* S, int64_t tr, const trf_state& st) {
    S[0] = st.ch.d1, S[tr] = st.ch.d2, S[2 * tr] = st.ch.e1, S[3 * tr] = st.ch.f1, S[4 * tr] = st.ch.f2;
    for (int c = 0; c < 3; ++c) {
        S[(5 + c) * tr] = st.ch.y1[c];
        S[(8 + c) * tr] = st.ch.y2[c];
        S[(12 + c) * tr] = st.a.z[c];
        S[(17 + c) * tr] = st.b.z[c];
    }
    S[11 * tr] = st.a.u, S[15 * tr] = st.a.since, S[16 * tr] = st.b.u, S[20 * tr] = st.b.since;
    S[21 * tr] = (double)st.n;
    S[22 * tr] = (double)st.seen;
}

// Row t of a prefix whose last row is t + to_end: trj_band reads t through (t >= 1), (t >= 2) and T - t only.
__device__ inline void trf_band(int64_t t, int to_end, const trf_args& p, double& a, double& b, double& c) {
    const int ts = (int)(t < 2 ? t : 2);
    trj_band(ts, ts + to_end + 1, p.lv, p.la, a, b, c);
}

__device__ inline bool trf_solvable(const trf_args& p, int64_t n, int seen) {
    return p.lv > 0.0 ? seen >= 1 : (n >= 3 ? seen >= 2 : (int64_t)seen == n);
}

__device__ inline double trf_next(double since) { return since < (double)TRJ_FAR ? since + 1.0 : (double)TRJ_FAR; }

// The two boundary rows n - 2 (st.a) and n - 1 (st.b) of the prefix of n >= 1 frames, on a copy of the chain.  With `gating` the
// newest frame's weight st.b.u is still its base weight: it is weighed against the prediction first (`seen` counts the frames before it).
__device__ inline void trf_boundary(trf_state& st, const trf_args& p, bool gating, int seen, double& ea, double* qa, double* qb) {
    trj_chain<3> pr = st.ch;
    double a, b, c, e, f;
    ea = 0.0;
    qa[0] = qa[1] = qa[2] = 0.0;
    if (st.n >= 2) {
        trf_band(st.n - 2, 1, p, a, b, c);
        const double rhs[3] = {st.a.u * st.a.z[0], st.a.u * st.a.z[1], st.a.u * st.a.z[2]};
        pr.step(a + st.a.u, b, c, rhs, ea, f, qa);
    }
    trf_band(st.n - 1, 0, p, a, b, c);
    if (gating) {
        trj_chain<3> g = pr;
        double pred[3];
        const double none[3] = {0.0, 0.0, 0.0};
        g.step(a, b, c, none, e, f, pred);
        const bool known = p.lv > 0.0 ? seen >= 1 : (st.n >= 3 && seen >= 2);       // trf_solvable of the prefix with w = 0 at its end
        const double r = trj_dist(pred, st.b.z);
        st.b.u = (known && st.b.u > 0.0 && r > p.gate) ? st.b.u * (p.gate / r) : st.b.u;
    }
    const double rhs[3] = {st.b.u * st.b.z[0], st.b.u * st.b.z[1], st.b.u * st.b.z[2]};
    pr.step(a + st.b.u, b, c, rhs, e, f, qb);
}

struct trf_out {
    float* pose;
    uint8_t* valid;
    float* residual;
    float* weight;
};

__device__ inline void trf_write(const trf_out& o, int64_t at, bool ok, const double* x, const double* z, double u, double gap, int max_gap) {
    for (int c = 0; c < 3; ++c) o.pose[at * 3 + c] = ok ? (float)x[c] : 0.0f;
    o.valid[at] = (ok && gap <= (double)max_gap) ? 1 : 0;
    o.residual[at] = (ok && u > 0.0) ? (float)trj_dist(x, z) : 0.0f;
    o.weight[at] = ok ? (float)u : 0.0f;
}

__device__ inline void trf_blank(const trf_out& o, int64_t at) {
    o.pose[at * 3] = o.pose[at * 3 + 1] = o.pose[at * 3 + 2] = 0.0f;
    o.valid[at] = 0;
    o.residual[at] = o.weight[at] = 0.0f;
}

// Back-substitution of the prefix of st.n >= 1 frames from its last row down: ALL = false walks lag + 1 rows and writes frame
// n - 1 - lag at `at` (the caller has checked that it exists); ALL = true walks lag rows and writes each, the last frame at `at`, earlier
// ones `step` elements before (rows before the stream's start are left to the caller).
template <bool ALL>
__device__ inline void trf_substitute(const trf_state& st, const double* S, const trf_args& p, double ea, const double* qa, const double* qb,
                                      const trf_out& o, int64_t at, int64_t step) {
    const int64_t tr = p.tracks;
    const bool ok = trf_solvable(p, st.n, st.seen);
    const int last = ALL ? p.lag - 1 : p.lag;
    double x1[3] = {0.0, 0.0, 0.0}, x2[3] = {0.0, 0.0, 0.0};
    double until = (double)TRJ_FAR;
    int r = p.lag > 0 ? (int)((st.n + (int64_t)p.lag - 3) % p.lag) : 0;             // row n - 3 of the ring (read where n >= 3 only)
    for (int i = 0; i <= last; ++i) {
        if (st.n - 1 - i < 0) break;
        const bool emit = ALL || i == last;
        double e, f, q[3], z[3] = {0.0, 0.0, 0.0}, u, since = 0.0;
        if (i == 0) {
            e = f = 0.0;
            u = st.b.u, since = st.b.since;
            for (int c = 0; c < 3; ++c) q[c] = qb[c], z[c] = st.b.z[c];
        } else if (i == 1) {
            e = ea, f = 0.0;
            u = st.a.u, since = st.a.since;
            for (int c = 0; c < 3; ++c) q[c] = qa[c], z[c] = st.a.z[c];
        } else {
            const double* R = S + (int64_t)(TRF_HEAD + TRF_ROW * r) * tr;
            e = R[0], f = R[tr], u = R[8 * tr];
            for (int c = 0; c < 3; ++c) q[c] = R[(2 + c) * tr];
            if (emit) {
                for (int c = 0; c < 3; ++c) z[c] = R[(5 + c) * tr];
                since = R[9 * tr];
            }
            r = r == 0 ? p.lag - 1 : r - 1;
        }
        double x[3];
        for (int c = 0; c < 3; ++c) x[c] = q[c] - e * x1[c] - f * x2[c];
        until = u > 0.0 ? 0.0 : trf_next(until);
        if (emit) trf_write(o, at - (ALL ? (int64_t)i * step : 0), ok, x, z, u, since < until ? since : until, p.max_gap);
        for (int c = 0; c < 3; ++c) {
            x2[c] = x1[c];
            x1[c] = x[c];
        }
    }
}

__global__ __launch_bounds__(64) void trajectory_filter_kernel(trj_args in, trf_args p, const uint8_t* reset, double* state, trf_out o,
                                                               int64_t* frame) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= p.tracks) return;
    const int C = in.T, J = in.J;
    const int64_t n = k / J, j = k - n * J;
    const int64_t base = n * C * J + j;                  // the track's frame c of this call is element base + c * J
    double* const S = state + k;
    // (no branch around the optional operand's load, as trj_fetch: without a reset the load goes to the pose and is selected away)
    const uint8_t flag = *(reset ? reset + n : (const uint8_t*)in.pose);
    trf_state st;
    trf_load(S, p.tracks, reset && flag != 0, st);
    trj_raw cur, nxt;
    trj_fetch(in, base, cur);
    for (int c = 0; c < C; ++c) {
        trj_fetch(in, base + (int64_t)trj_min(c + 1, C - 1) * J, nxt);
        trj_frame f;
        trj_decode(cur, f);
        const int64_t t = st.n;
        if (t >= 2) {                                    // row t - 2 is final: interior coefficients
            double a, b, cc, e, ff, q[3];
            trf_band(t - 2, 2, p, a, b, cc);
            const double rhs[3] = {st.a.u * st.a.z[0], st.a.u * st.a.z[1], st.a.u * st.a.z[2]};
            st.ch.step(a + st.a.u, b, cc, rhs, e, ff, q);
            if (p.lag > 0) {
                double* R = S + (int64_t)(TRF_HEAD + TRF_ROW * (int)((t - 2) % p.lag)) * p.tracks;
                R[0] = e, R[p.tracks] = ff, R[8 * p.tracks] = st.a.u, R[9 * p.tracks] = st.a.since;
                for (int i = 0; i < 3; ++i) R[(2 + i) * p.tracks] = q[i], R[(5 + i) * p.tracks] = st.a.z[i];
            }
        }
        const int before = st.seen;
        st.a = st.b;
        st.b.u = f.w;
        for (int i = 0; i < 3; ++i) st.b.z[i] = f.z[i];
        st.b.since = f.w > 0.0 ? 0.0 : (t == 0 ? (double)TRJ_FAR : trf_next(st.a.since));
        st.n = t + 1;
        st.seen = trj_min(before + (f.w > 0.0 ? 1 : 0), 2);
        double ea, qa[3], qb[3];
        trf_boundary(st, p, p.gate > 0.0, before, ea, qa, qb);
        const int64_t at = base + (int64_t)c * J;
        if (t >= p.lag) trf_substitute<false>(st, S, p, ea, qa, qb, o, at, 0);
        else trf_blank(o, at);
        if (j == 0) frame[n * C + c] = t >= p.lag ? t - p.lag : -1;
        cur = nxt;
    }
    trf_store(S, p.tracks, st);
}

__global__ __launch_bounds__(64) void trajectory_filter_tail_kernel(trf_args p, int J, const double* state, trf_out o, int64_t* frame) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= p.tracks) return;
    const int64_t n = k / J, j = k - n * J;
    const double* const S = state + k;
    trf_state st;
    trf_load(S, p.tracks, false, st);
    const int64_t end = (n * p.lag + (p.lag - 1)) * J + j;      // the last row: frame st.n - 1
    if (st.n >= 1) {
        double ea, qa[3], qb[3];
        trf_boundary(st, p, false, 0, ea, qa, qb);
        trf_substitute<true>(st, S, p, ea, qa, qb, o, end, J);
    }
    for (int i = 0; i < p.lag; ++i) {                    // row lag - 1 - i is frame st.n - 1 - i
        if (st.n - 1 - i < 0) trf_blank(o, end - (int64_t)i * J);
        if (j == 0) frame[n * p.lag + (p.lag - 1 - i)] = st.n - 1 - i >= 0 ? st.n - 1 - i : -1;
    }
}

inline bool trf_shape_ok(int32_t N, int32_t C, int32_t J, int32_t lag, float lv, float la, int32_t max_gap) {
    if (lag < 0 || lag > TRF_MAX_LAG || max_gap < 0) return false;
    if (!trj_shape_ok(N, C, J, lv, la)) return false;
    return (int64_t)N * J * (TRF_HEAD + TRF_ROW * lag) < ((int64_t)1 << 31);
}

inline trf_args trf_pack(int32_t N, int32_t J, int32_t lag, float lv, float la, float gate, int32_t max_gap) {
    trf_args p;
    p.lv = (double)lv;
    p.la = (double)la;
    p.gate = (double)gate;
    p.lag = lag;
    p.max_gap = max_gap;
    p.tracks = (int64_t)N * J;
    return p;
}

}  // namespace

extern "C" int64_t egr_trajectory_filter_state_slots(int32_t lag) {
    return lag < 0 || lag > TRF_MAX_LAG ? (int64_t)EGR_EINVAL : (int64_t)(TRF_HEAD + TRF_ROW * lag);
}

extern "C" int egr_trajectory_filter_f32(const float* pose, const float* weight, const uint8_t* obs, const uint8_t* reset, double* state,
                                         int32_t N, int32_t C, int32_t J, int32_t lag, float vel_weight, float accel_weight, float gate,
                                         int32_t max_gap, float* pose_out, uint8_t* valid, float* residual, float* weight_out, int64_t* frame,
                                         void* stream) {
    if (!pose || !state || !pose_out || !valid || !residual || !weight_out || !frame) return EGR_ENULL;
    if (!trf_shape_ok(N, C, J, lag, vel_weight, accel_weight, max_gap) || !trj_number(gate)) return EGR_EINVAL;
    const trj_args in = trj_pack(pose, weight, obs, N, C, J, vel_weight, accel_weight, 0.0f, 0, max_gap);
    const trf_args p = trf_pack(N, J, lag, vel_weight, accel_weight, gate, max_gap);
    const trf_out o = {pose_out, valid, residual, weight_out};
    hipLaunchKernelGGL(trajectory_filter_kernel, dim3((unsigned)((p.tracks + 63) / 64)), dim3(64), 0, (hipStream_t)stream, in, p, reset, state,
                       o, frame);
    return egr_launch_status();
}

extern "C" int egr_trajectory_filter_tail_f32(const double* state, int32_t N, int32_t J, int32_t lag, float vel_weight, float accel_weight,
                                              int32_t max_gap, float* pose_out, uint8_t* valid, float* residual, float* weight_out,
                                              int64_t* frame, void* stream) {
    if (!state || !pose_out || !valid || !residual || !weight_out || !frame) return EGR_ENULL;
    if (!trf_shape_ok(N, 1, J, lag, vel_weight, accel_weight, max_gap)) return EGR_EINVAL;
    if (lag == 0) return 0;                              // no rows
    const trf_args p = trf_pack(N, J, lag, vel_weight, accel_weight, 0.0f, max_gap);
    const trf_out o = {pose_out, valid, residual, weight_out};
    hipLaunchKernelGGL(trajectory_filter_tail_kernel, dim3((unsigned)((p.tracks + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p, J, state, o,
                       frame);
    return egr_launch_status();
}
