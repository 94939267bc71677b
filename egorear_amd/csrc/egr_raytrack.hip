// Ray-space clip smoothing: the 3-D tracks of a clip fitted to the views' rays directly.  A track is one joint of one
// clip, T frames; with G_t = sum_v w_tv R^T P R and g_t = -sum_v w_tv R^T P t the normal equations of frame t's rays (egr_rays.h) its
// positions solve
//   (blockdiag(G_t) + (lv D1^T D1 + la D2^T D2) (x) I_3) x = (g_t)
// - symmetric, block pentadiagonal with 3 x 3 blocks, the off-diagonal blocks multiples of the identity.  With huber = delta > 0 the
// solve is repeated K = reweights more times with the ray weights w_tv min(1, delta / dist_tv) of the previous solution (IRLS).
//
// Two kernels:
//   ray_track_rays_kernel   a thread per (frame, joint): the trigonometry of its V rays, once - d[3] and w in fp64, planes of T x tracks
//                           laid out (view, slot, t, track), so that the solve's reads at one t coalesce over the tracks
//   ray_track_solve_kernel  one lane per track, the tracks of a clip in adjacent lanes.  A block LDL^T along t in fp64 without pivoting:
//                             D_t = G_t + a_t I - E_{t-1} D_{t-1} E_{t-1}^T - F_{t-2} D_{t-2} F_{t-2}^T,     (a, b, c)_t = trj_band
//                             E_t = M_t D_t^-1,  M_t = b_t I - c_{t-1} E_{t-1}^T,     F_t = c_t D_t^-1
//                           (F_{t-1} D_{t-1} = c_{t-1} I, so E_{t-1} D_{t-1} E_{t-1}^T = E_{t-1} M_{t-1}^T and F D F^T = c^2 D^-1: the sweep
//                           carries D^-1 of two frames, M and E of one, c of two and two reduced right-hand sides).  Every D_t is
//                           factored by the 3 x 3 LDL^T of rays::factor; its three d are the scalar pivots of the solvability rule.  E_t
//                           (9), D_t^-1 (6) and q_t = D_t^-1 y_t (3) go to an fp64 workspace laid out (slot, t, track); the backward
//                           sweep substitutes x_t = q_t - E_t^T x_{t+1} - c_t D_t^-1 x_{t+2} and leaves x_t in the q slots, where the next
//                           reweighted solve and the energy pass read it.  The operands of the next chunk of frames are fetched before
//                           this chunk's steps are computed, as in egr_trajectory.hip.  Every sweep of the K + 1 solves and the energy
//                           pass run inside the one launch.
// No atomics, no LDS, no cross-lane traffic, a fixed order everywhere: a track's bits depend on its own operands only.
#include "egr_block_band.h"      // rt_chain, rt_sym_vec: the block elimination, shared with egr_infotrack.hip
#include "egr_rays.h"
#include "egr_trajectory_band.h"

namespace {

constexpr int RT_MAX_T = 4096, RT_MAX_REWEIGHTS = 16;
constexpr int RT_RAY_SLOTS = 4;                                    // d[3], w of one view
constexpr int RT_E = 0, RT_DINV = 9, RT_Q = 15, RT_SOLVE_SLOTS = 18;
// Frames whose operands are in flight together, forward and backward.  The forward sweep carries D^-1 of two frames, M, E, two right-hand
// sides and forms a frame's block from up to four rays: with two frames of rays in flight each way it does not fit the 512 registers
// of a lane (276 bytes of scratch), with one it does (DESIGN.md 5u has the compiler's figures).
constexpr int RT_CH_FWD = 1, RT_CH_BWD = 2;
constexpr int RT_FAR = 1 << 30;

struct rt_args {
    const float* cams;
    const float* ctm;            // nullable: the syn rig
    int T, V, J;
    int64_t tracks;
    double lv, la, delta, min_pivot_ratio;
    int reweights, max_gap;
};

__host__ __device__ inline int rt_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int rt_max(int a, int b) { return a > b ? a : b; }

// ---- the ray pass: thread i = t * tracks + (n J + j)
__host__ __device__ inline void rt_rays_one(const float* coords, const float* conf, const float* cams, int T, int V, int J, int64_t tracks,
                                            float sx, float sy, float thr, int64_t i, double* ws) {
    const int64_t plane = (int64_t)T * tracks;
    const int64_t t = i / tracks, k = i - t * tracks, n = k / J, j = k - n * J;
    for (int v = 0; v < V; ++v) {
        rays::ray ry;
        rays::make_ray(coords, conf, cams + v * rays::REC, ((n * T + t) * V + v) * J + j, (double)sx, (double)sy, thr, ry);
        for (int c = 0; c < 3; ++c) ws[(int64_t)(v * RT_RAY_SLOTS + c) * plane + i] = ry.d[c];
        ws[(int64_t)(v * RT_RAY_SLOTS + 3) * plane + i] = ry.w;
    }
}

// the rays of one frame of one track, as the ray pass left them (a view past V reads view V - 1, a valid address, and weighs nothing)
struct rt_rays {
    double d[rays::MAX_V][3], w[rays::MAX_V];
};

__host__ __device__ inline void rt_fetch(const rt_args& p, const double* rw, int64_t plane, int64_t row, rt_rays& o) {
#pragma unroll
    for (int v = 0; v < rays::MAX_V; ++v) {
        const int vv = rt_min(v, p.V - 1);
        for (int c = 0; c < 3; ++c) o.d[v][c] = rw[(int64_t)(vv * RT_RAY_SLOTS + c) * plane + row];
        o.w[v] = rw[(int64_t)(vv * RT_RAY_SLOTS + 3) * plane + row];
    }
}

// distance of x from the ray d of the view with extrinsics (R, t): |P (R x + t)|
__host__ __device__ inline double rt_dist(const double* R, const double* t, const double* d, const double* x) {
    double q[3];
    rays::apply(R, t, x, q);
    const double dq = d[0] * q[0] + d[1] * q[1] + d[2] * q[2];
    const double r0 = q[0] - d[0] * dq, r1 = q[1] - d[1] * dq, r2 = q[2] - d[2] * dq;
    return sqrt(r0 * r0 + r1 * r1 + r2 * r2);
}

// every output of a track that is not solvable
__host__ __device__ inline void rt_dead(const rt_args& p, int64_t n, int64_t j, int64_t k, float* pose, uint8_t* valid, float* residual,
                                        float* weight, uint8_t* nrays, float* energy) {
    for (int t = 0; t < p.T; ++t) {
        const int64_t b = n * p.T + t, at = b * p.J + j;
        pose[at * 3] = pose[at * 3 + 1] = pose[at * 3 + 2] = 0.0f;
        valid[at] = 0;
        nrays[at] = 0;
        for (int v = 0; v < p.V; ++v) residual[(b * p.V + v) * p.J + j] = weight[(b * p.V + v) * p.J + j] = 0.0f;
    }
    energy[k] = 0.0f;
}

__host__ __device__ inline void rt_solve_one(const rt_args& p, int64_t k, double* ws, float* pose, uint8_t* valid, float* residual,
                                             float* weight, uint8_t* nrays, float* energy) {
    const int T = p.T, J = p.J, V = p.V;
    const int64_t n = k / J, j = k - n * J;
    const int64_t plane = (int64_t)T * p.tracks;                     // one workspace slot
    const double* const rw = ws + k;                                 // slot s of view v at frame t: rw[(v * 4 + s) * plane + t * tracks]
    double* const S = ws + (int64_t)V * RT_RAY_SLOTS * plane + k;    // slot s of frame t: S[s * plane + t * tracks]
    for (int it = 0; it <= p.reweights; ++it) {
        const bool first = it == 0, last = it == p.reweights;
        // ---- forward sweep: form every frame's block from its rays, factor, reduce the right-hand side
        {
            constexpr int CH = RT_CH_FWD;
            rt_chain ch;
            rt_rays cur[CH], nxt[CH];
            double xp[CH][3], xn[CH][3];                             // the previous solve's x_t, read from the q slots before they are overwritten
            int used_rays = 0, used_frames = 0, full_frames = 0, since = RT_FAR;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int64_t row = (int64_t)rt_min(i, T - 1) * p.tracks;
                rt_fetch(p, rw, plane, row, cur[i]);
                for (int c = 0; c < 3; ++c) xp[i][c] = S[(RT_Q + c) * plane + row];       // (not used by the first sweep)
            }
            for (int t0 = 0; t0 < T; t0 += CH) {
#pragma unroll
                for (int i = 0; i < CH; ++i) {                       // (rows ahead of every row this chunk writes; past the end the last row, unused)
                    const int64_t row = (int64_t)rt_min(t0 + CH + i, T - 1) * p.tracks;
                    rt_fetch(p, rw, plane, row, nxt[i]);
                    for (int c = 0; c < 3; ++c) xn[i][c] = S[(RT_Q + c) * plane + row];
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int t = t0 + i;
                    if (t < T) {
                        const int64_t b = n * T + t;
                        rays::normal_eq g;
                        int count = 0;
#pragma unroll
                        for (int v = 0; v < rays::MAX_V; ++v) {
                            const int vv = rt_min(v, V - 1);
                            const double w0 = v < V ? cur[i].w[v] : 0.0;
                            double R[9], tr[3], w = w0;
                            rays::extrinsics(p.cams + vv * rays::REC, p.ctm, b * V + vv, R, tr);
                            if (!first && w0 > 0.0) {
                                const double r = rt_dist(R, tr, cur[i].d[v], xp[i]);
                                w = r > p.delta ? w0 * (p.delta / r) : w0;
                            }
                            rays::add_ray(R, tr, cur[i].d[v], w, g);
                            count += w0 > 0.0 ? 1 : 0;
                            if (last && v < V) weight[(b * V + v) * J + j] = (float)w;
                        }
                        double a, bb, c, E[9], Di[6], q[3];
                        trj_band(t, T, p.lv, p.la, a, bb, c);
                        ch.step(g, a, bb, c, E, Di, q);
                        const int64_t row = (int64_t)t * p.tracks;
                        for (int s = 0; s < 9; ++s) S[(RT_E + s) * plane + row] = E[s];
                        for (int s = 0; s < 6; ++s) S[(RT_DINV + s) * plane + row] = Di[s];
                        for (int s = 0; s < 3; ++s) S[(RT_Q + s) * plane + row] = q[s];
                        used_rays += count;
                        used_frames += count >= 1 ? 1 : 0;
                        full_frames += count >= 2 ? 1 : 0;
                        if (last) {
                            since = count > 0 ? 0 : (since < RT_FAR ? since + 1 : RT_FAR);
                            valid[b * J + j] = since <= p.max_gap ? 1 : 0;
                            nrays[b * J + j] = (uint8_t)count;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    cur[i] = nxt[i];
                    for (int c = 0; c < 3; ++c) xp[i][c] = xn[i][c];
                }
            }
            if (first) {
                // solvable: (a) enough rays for the penalty's null space, (b) no scalar pivot at or below the ratio of the largest
                // diagonal entry (include/egorear_hip.h; a NaN anywhere fails)
                const bool enough = p.lv > 0.0 ? used_rays >= 2 : (T >= 3 ? used_rays >= 3 && used_frames >= 2 : full_frames == T);
                if (!(enough && ch.finite && ch.min_pivot > p.min_pivot_ratio * ch.max_diag)) {
                    rt_dead(p, n, j, k, pose, valid, residual, weight, nrays, energy);
                    return;
                }
            }
        }
        // ---- backward sweep: substitute; x_t goes to the q slots, the last one writes the pose too
        constexpr int CH = RT_CH_BWD;
        double x1[3] = {0.0, 0.0, 0.0}, x2[3] = {0.0, 0.0, 0.0};
        double cs[CH][RT_SOLVE_SLOTS], ns[CH][RT_SOLVE_SLOTS];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int64_t row = (int64_t)rt_max(T - 1 - i, 0) * p.tracks;
            for (int s = 0; s < RT_SOLVE_SLOTS; ++s) cs[i][s] = S[s * plane + row];
        }
        for (int t1 = T - 1; t1 >= 0; t1 -= CH) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {                           // (rows below every row this chunk writes; past the start row 0, unused)
                const int64_t row = (int64_t)rt_max(t1 - CH - i, 0) * p.tracks;
                for (int s = 0; s < RT_SOLVE_SLOTS; ++s) ns[i][s] = S[s * plane + row];
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int t = t1 - i;
                if (t >= 0) {
                    double a, bb, c, fx[3], x[3];
                    trj_band(t, T, p.lv, p.la, a, bb, c);
                    const double* E = cs[i] + RT_E;
                    rt_sym_vec(cs[i] + RT_DINV, x2, fx);
                    for (int r = 0; r < 3; ++r) x[r] = cs[i][RT_Q + r] - (E[r] * x1[0] + E[3 + r] * x1[1] + E[6 + r] * x1[2]) - c * fx[r];
                    const int64_t row = (int64_t)t * p.tracks;
                    for (int r = 0; r < 3; ++r) S[(RT_Q + r) * plane + row] = x[r];
                    if (last)
                        for (int r = 0; r < 3; ++r) pose[((n * T + t) * J + j) * 3 + r] = (float)x[r];
                    for (int r = 0; r < 3; ++r) {
                        x2[r] = x1[r];
                        x1[r] = x[r];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < CH; ++i)
                for (int s = 0; s < RT_SOLVE_SLOTS; ++s) cs[i][s] = ns[i][s];
        }
    }
    // ---- energy pass, from the last frame down: no chain - the rays' distances at x_t, the penalties, the other half of the validity
    double e_data = 0.0, e_vel = 0.0, e_acc = 0.0, x1[3] = {0.0, 0.0, 0.0}, x2[3] = {0.0, 0.0, 0.0};
    int until = RT_FAR;
#pragma unroll 2
    for (int t = T - 1; t >= 0; --t) {
        const int64_t row = (int64_t)t * p.tracks, b = n * T + t;
        rt_rays ry;
        rt_fetch(p, rw, plane, row, ry);
        const double x[3] = {S[RT_Q * plane + row], S[(RT_Q + 1) * plane + row], S[(RT_Q + 2) * plane + row]};
        int count = 0;
#pragma unroll
        for (int v = 0; v < rays::MAX_V; ++v) {
            const int vv = rt_min(v, V - 1);
            const double w0 = v < V ? ry.w[v] : 0.0;
            double R[9], tr[3];
            rays::extrinsics(p.cams + vv * rays::REC, p.ctm, b * V + vv, R, tr);
            const double r = w0 > 0.0 ? rt_dist(R, tr, ry.d[v], x) : 0.0;
            e_data += w0 * (p.delta > 0.0 && r > p.delta ? 2.0 * p.delta * r - p.delta * p.delta : r * r);
            count += w0 > 0.0 ? 1 : 0;
            if (v < V) residual[(b * V + v) * J + j] = (float)r;
        }
        if (t < T - 1) {
            const double v0 = x1[0] - x[0], v1 = x1[1] - x[1], v2 = x1[2] - x[2];
            e_vel += v0 * v0 + v1 * v1 + v2 * v2;
        }
        if (t < T - 2) {
            const double a0 = x2[0] - 2.0 * x1[0] + x[0], a1 = x2[1] - 2.0 * x1[1] + x[1], a2 = x2[2] - 2.0 * x1[2] + x[2];
            e_acc += a0 * a0 + a1 * a1 + a2 * a2;
        }
        until = count > 0 ? 0 : (until < RT_FAR ? until + 1 : RT_FAR);
        if (until <= p.max_gap) valid[b * J + j] = 1;                // (the forward sweep wrote the flag of the frames before t)
        for (int r = 0; r < 3; ++r) {
            x2[r] = x1[r];
            x1[r] = x[r];
        }
    }
    energy[k] = (float)(e_data + p.lv * e_vel + p.la * e_acc);
}

__global__ __launch_bounds__(128) void ray_track_rays_kernel(const float* coords, const float* conf, const float* cams, int T, int V, int J,
                                                             int64_t tracks, float sx, float sy, float thr, double* ws) {
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= (int64_t)T * tracks) return;
    rt_rays_one(coords, conf, cams, T, V, J, tracks, sx, sy, thr, i, ws);
}

__global__ __launch_bounds__(64) void ray_track_solve_kernel(rt_args p, double* ws, float* pose, uint8_t* valid, float* residual, float* weight,
                                                             uint8_t* nrays, float* energy) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= p.tracks) return;
    rt_solve_one(p, k, ws, pose, valid, residual, weight, nrays, energy);
}

inline bool rt_number(float v) { return v >= 0.0f && v <= 3.402823466e38f; }       // non-negative and finite

inline bool rt_shape_ok(int32_t N, int32_t T, int32_t V, int32_t J) {
    return N >= 1 && J >= 1 && V >= 2 && V <= rays::MAX_V && T >= 1 && T <= RT_MAX_T && (int64_t)N * T * V * J * 2 < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int64_t egr_ray_track_workspace_bytes(int32_t N, int32_t T, int32_t V, int32_t J) {
    if (!rt_shape_ok(N, T, V, J)) return 0;
    return (int64_t)(V * RT_RAY_SLOTS + RT_SOLVE_SLOTS) * T * N * J * (int64_t)sizeof(double);
}

extern "C" int egr_ray_track_f32(const float* coords, const float* conf, const float* cams, const float* ctm, int32_t N, int32_t T, int32_t V,
                                 int32_t J, float sx, float sy, float threshold, float vel_weight, float accel_weight, float huber,
                                 int32_t reweights, int32_t max_gap, double min_pivot_ratio, double* workspace, int64_t workspace_bytes,
                                 float* pose, uint8_t* valid, float* residual, float* weight, uint8_t* nrays, float* energy, void* stream) {
    if (!coords || !conf || !cams || !workspace || !pose || !valid || !residual || !weight || !nrays || !energy) return EGR_ENULL;
    if (!rt_shape_ok(N, T, V, J)) return EGR_EINVAL;
    if (!(sx > 0.f && sx <= 3.0e38f && sy > 0.f && sy <= 3.0e38f && threshold == threshold)) return EGR_EINVAL;
    if (!rt_number(vel_weight) || !rt_number(accel_weight) || !(vel_weight > 0.0f || accel_weight > 0.0f)) return EGR_EINVAL;
    if (!rt_number(huber) || reweights < 0 || reweights > RT_MAX_REWEIGHTS || (reweights > 0) != (huber > 0.0f) || max_gap < 0)
        return EGR_EINVAL;
    if (!(min_pivot_ratio >= 0.0 && min_pivot_ratio < 1.0)) return EGR_EINVAL;
    if (workspace_bytes < egr_ray_track_workspace_bytes(N, T, V, J)) return EGR_EWORKSPACE;
    rt_args p;
    p.cams = cams;
    p.ctm = ctm;
    p.T = T;
    p.V = V;
    p.J = J;
    p.tracks = (int64_t)N * J;
    p.lv = (double)vel_weight;
    p.la = (double)accel_weight;
    p.delta = (double)huber;
    p.min_pivot_ratio = min_pivot_ratio;
    p.reweights = reweights;
    p.max_gap = max_gap;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cells = (int64_t)T * p.tracks;
    hipLaunchKernelGGL(ray_track_rays_kernel, dim3((unsigned)((cells + 127) / 128)), dim3(128), 0, s, coords, conf, cams, T, V, J, p.tracks, sx,
                       sy, threshold, workspace);
    hipLaunchKernelGGL(ray_track_solve_kernel, dim3((unsigned)((p.tracks + 63) / 64)), dim3(64), 0, s, p, workspace, pose, valid, residual,
                       weight, nrays, energy);
    return egr_launch_status();
}
