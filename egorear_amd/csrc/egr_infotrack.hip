// Information-weighted clip smoothing: the 3 x 3 information matrix of a 3-D point under the views that see it, and
// the clip smoother that takes one such matrix a frame instead of a scalar weight.
//
//   joint_info_kernel    a thread per (frame, joint).  W = sum_v conf_v J_v^T J_v, J_v the 2 x 3 Jacobian of view v's fisheye projection
//                        (in the units of `coords`) at the point: analytic, fp64 on the fp32 operands.  With q = R p + t, n = |q_xy|,
//                        e = q_xy / n, theta = atan2(-q_z, n), r^2 = n^2 + q_z^2 and rho(theta) the W2C polynomial
//                          d pixel / d q = rho/n (I_2 - e e^T) [I_2 0] + rho' e (q_z e_x, q_z e_y, -n) / r^2,
//                        the rows divided by (sx W_img, sy H_img), times R.  A fixed order over the views, no atomics.
//   info_track_kernel    one lane per track, the tracks of a clip in adjacent lanes.  A track minimises
//                          sum_t s_t (x_t - z_t)^T W_t (x_t - z_t) + lv sum |x_{t+1} - x_t|^2 + la sum |x_{t+1} - 2 x_t + x_{t-1}|^2
//                        : the system of egr_raytrack.hip with G_t = s_t W_t, g_t = s_t W_t z_t, eliminated by the same rt_chain
//                        (egr_block_band.h) into the same (slot, t, track) fp64 workspace - E (9), D^-1 (6), q (3).  It is solved
//                        for the displacement d_t = x_t - z_t (z_t = 0 in a gap): (blockdiag(s W) + P) d = -P z with P the penalty,
//                        whatever s - the unknowns are the size of the noise, not of the distance from the device, a frame that no
//                        penalty couples to its neighbours comes back exactly (d = 0), and r_t = sqrt(d^T W d) needs no difference.
//                        The operands of the frames two chunks ahead are fetched before this chunk's steps are computed.  Every
//                        sweep of the K + 1 solves and the output pass run inside the one launch.
// No LDS, no cross-lane traffic, a fixed order everywhere: an output's bits depend on its own operands only.
#include "egr_block_band.h"
#include "egr_rays.h"
#include "egr_trajectory_band.h"

namespace {

constexpr int IT_MAX_T = 4096, IT_MAX_REWEIGHTS = 16;
constexpr int IT_E = 0, IT_DINV = 9, IT_Q = 15, IT_SOLVE_SLOTS = 18;
// Frames of a chunk, forward and backward.  A frame's operands are ten floats and a flag (a ray-track frame is sixteen doubles), so the
// forward sweep's three chunks of two frames and the backward sweep's two fit without scratch (DESIGN.md 5v has the compiler's figures).
constexpr int IT_CH_FWD = 2, IT_CH_BWD = 2;
constexpr int IT_FAR = 1 << 30;

__host__ __device__ inline int it_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int it_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline bool it_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// ---- the information matrix: thread i = b J + j
__host__ __device__ inline void ji_one(const float* points, const float* conf, const float* cams, const float* ctm, int V, int J, double sx,
                                       double sy, float thr, double min_det_ratio, int64_t i, float* info, uint8_t* views, float* sigma,
                                       uint8_t* valid) {
    const int64_t b = i / J, j = i - b * J;
    const float pf[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    const bool point = it_finite(pf[0]) && it_finite(pf[1]) && it_finite(pf[2]);
    const double p[3] = {point ? (double)pf[0] : 0.0, point ? (double)pf[1] : 0.0, point ? (double)pf[2] : 0.0};
    rays::normal_eq w;
    int count = 0;
    for (int v = 0; v < V; ++v) {
        const float* cam = cams + v * rays::REC;
        const float cf = conf[(b * V + v) * J + j];
        double R[9], t[3], q[3];
        rays::extrinsics(cam, ctm, b * V + v, R, t);
        rays::apply(R, t, p, q);
        const double n2 = q[0] * q[0] + q[1] * q[1], n = sqrt(n2), r2 = n2 + q[2] * q[2];
        // make_ray's rule for the confidence; the point gives a pixel off the optical axis (n > 0; a NaN in R or t fails it)
        const bool use = point && cf >= thr && cf > 0.f && isfinite(cf) && n > 0.0 && r2 <= 1.7e308;
        if (!use) continue;
        const double theta = atan2(-q[2], n);
        const int nw = rays::w2c_degree(cam);
        double rho = 0.0, drho = 0.0;
        for (int k = nw - 1; k >= 0; --k) {
            drho = drho * theta + rho;
            rho = rho * theta + (double)cam[rays::W2C + k];
        }
        const double ex = q[0] / n, ey = q[1] / n, rn = rho / n, dr = drho / r2;
        const double ku = 1.0 / (sx * (double)cam[3]), kv = 1.0 / (sy * (double)cam[4]);
        // rows of d coords / d q
        const double ju[3] = {ku * (rn * ey * ey + dr * q[2] * ex * ex), ku * (-rn * ex * ey + dr * q[2] * ex * ey), ku * (-dr * n * ex)};
        const double jv[3] = {kv * (-rn * ex * ey + dr * q[2] * ex * ey), kv * (rn * ex * ex + dr * q[2] * ey * ey), kv * (-dr * n * ey)};
        // ... times R: rows of d coords / d p
        double a[3], c[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = ju[0] * R[k] + ju[1] * R[3 + k] + ju[2] * R[6 + k];
            c[k] = jv[0] * R[k] + jv[1] * R[3 + k] + jv[2] * R[6 + k];
        }
        const double cw = (double)cf;
        w.a00 += cw * (a[0] * a[0] + c[0] * c[0]);
        w.a01 += cw * (a[0] * a[1] + c[0] * c[1]);
        w.a02 += cw * (a[0] * a[2] + c[0] * c[2]);
        w.a11 += cw * (a[1] * a[1] + c[1] * c[1]);
        w.a12 += cw * (a[1] * a[2] + c[1] * c[2]);
        w.a22 += cw * (a[2] * a[2] + c[2] * c[2]);
        ++count;
    }
    rays::ldl f;
    const bool ok = count > 0 && rays::factor(w, min_det_ratio, f);
    double tr = 0.0;
    if (ok) {
        const double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
        double k0[3], k1[3], k2[3];
        rays::ldl_solve(f, e0, k0);
        rays::ldl_solve(f, e1, k1);
        rays::ldl_solve(f, e2, k2);
        tr = k0[0] + k1[1] + k2[2];
    }
    float* o = info + i * 6;
    o[0] = (float)w.a00;
    o[1] = (float)w.a01;
    o[2] = (float)w.a02;
    o[3] = (float)w.a11;
    o[4] = (float)w.a12;
    o[5] = (float)w.a22;
    views[i] = (uint8_t)count;
    sigma[i] = ok ? (float)sqrt(tr) : 0.0f;
    valid[i] = ok ? 1 : 0;
}

// ---- the smoother
struct it_args {
    const float* pose;
    const float* info;
    const uint8_t* obs;          // nullable: every frame
    int T, J;
    int64_t tracks;
    double lv, la, delta, min_pivot_ratio;
    int reweights, max_gap;
};

// What one frame's loads return, before any arithmetic: a chunk of them is in flight together.  (No branch on the optional mask: without
// one the load goes to the frame's pose - an address that is valid - and its value is selected away, as in egr_trajectory.hip.)
struct it_raw {
    float z[3], w[6];
    uint8_t on;
};

struct it_frame {
    double z[3], w[6];           // zeros for a frame that is not used: what stands there is selected away, not multiplied
    bool used;
};

__host__ __device__ inline void it_fetch(const it_args& p, int64_t at, it_raw& r) {
    const float* xyz = p.pose + at * 3;
    const float* m = p.info + at * 6;
    const uint8_t on = *(p.obs ? p.obs + at : (const uint8_t*)xyz);
    r.on = p.obs ? on : (uint8_t)1;
    for (int c = 0; c < 3; ++c) r.z[c] = xyz[c];
    for (int c = 0; c < 6; ++c) r.w[c] = m[c];
}

__host__ __device__ inline void it_decode(const it_raw& r, it_frame& o) {
    bool on = r.on != 0 && it_finite(r.z[0]) && it_finite(r.z[1]) && it_finite(r.z[2]);
    for (int c = 0; c < 6; ++c) on = on && it_finite(r.w[c]);
    on = on && r.w[0] >= 0.0f && r.w[3] >= 0.0f && r.w[5] >= 0.0f && (double)r.w[0] + (double)r.w[3] + (double)r.w[5] > 0.0;
    o.used = on;
    for (int c = 0; c < 3; ++c) o.z[c] = on ? (double)r.z[c] : 0.0;
    for (int c = 0; c < 6; ++c) o.w[c] = on ? (double)r.w[c] : 0.0;
}

// the displacement d = x - z in coordinate units: sqrt(d^T W d), 0 where rounding leaves the form negative
__host__ __device__ inline double it_norm(const it_frame& o, const double* d) {
    double wd[3];
    rt_sym_vec(o.w, d, wd);
    const double r2 = d[0] * wd[0] + d[1] * wd[1] + d[2] * wd[2];
    return r2 > 0.0 ? sqrt(r2) : 0.0;
}

// every output of a track that is not solvable
__host__ __device__ inline void it_dead(const it_args& p, int64_t base, int64_t k, float* pose, uint8_t* valid, float* residual, float* weight,
                                        float* energy) {
    for (int t = 0; t < p.T; ++t) {
        const int64_t at = base + (int64_t)t * p.J;
        pose[at * 3] = pose[at * 3 + 1] = pose[at * 3 + 2] = 0.0f;
        valid[at] = 0;
        residual[at] = weight[at] = 0.0f;
    }
    energy[k] = 0.0f;
}

__host__ __device__ inline void it_solve_one(const it_args& p, int64_t k, double* ws, float* pose, uint8_t* valid, float* residual, float* weight,
                                             float* energy) {
    const int T = p.T, J = p.J;
    const int64_t n = k / J, j = k - n * J;
    const int64_t base = n * T * J + j;                              // the track's frame t is element base + t * J
    const int64_t plane = (int64_t)T * p.tracks;                     // one workspace slot
    double* const S = ws + k;                                        // slot s of frame t: S[s * plane + t * tracks]
    for (int it = 0; it <= p.reweights; ++it) {
        const bool first = it == 0, last = it == p.reweights;
        // ---- forward sweep: every frame's block from its matrix, the right-hand side -(P z)_t from the frames two either side, factor,
        // reduce.  Three chunks of operands are held: this one, the next - both arrived, row t reads z of t + 1 and t + 2 - and the one
        // after, in flight.
        {
            constexpr int CH = IT_CH_FWD;
            static_assert(CH >= 2, "row t reads the frames t + 1 and t + 2 from this chunk and the next");
            rt_chain ch;
            it_raw cur[CH], nxt[CH], far[CH];
            double dp[CH][3], dn[CH][3];                             // the previous solve's d_t, read from the q slots before they are overwritten
            double zp1[3] = {0.0, 0.0, 0.0}, zp2[3] = {0.0, 0.0, 0.0}, bp1 = 0.0, cp1 = 0.0, cp2 = 0.0;      // z and the band of t - 1, t - 2
            int used_frames = 0, since = IT_FAR;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int tt = it_min(i, T - 1);
                it_fetch(p, base + (int64_t)tt * J, cur[i]);
                it_fetch(p, base + (int64_t)it_min(CH + i, T - 1) * J, nxt[i]);
                for (int c = 0; c < 3; ++c) dp[i][c] = S[(IT_Q + c) * plane + (int64_t)tt * p.tracks];       // (not used by the first sweep)
            }
            for (int t0 = 0; t0 < T; t0 += CH) {
#pragma unroll
                for (int i = 0; i < CH; ++i) {                       // (rows ahead of every row this chunk writes; past the end the last row, unused)
                    it_fetch(p, base + (int64_t)it_min(t0 + 2 * CH + i, T - 1) * J, far[i]);
                    const int tt = it_min(t0 + CH + i, T - 1);
                    for (int c = 0; c < 3; ++c) dn[i][c] = S[(IT_Q + c) * plane + (int64_t)tt * p.tracks];
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int t = t0 + i;
                    if (t < T) {
                        it_frame o, o1, o2;
                        it_decode(cur[i], o);
                        it_decode(i + 1 < CH ? cur[(i + 1) % CH] : nxt[(i + 1) % CH], o1);       // (past the end: the band's entries are 0)
                        it_decode(i + 2 < CH ? cur[(i + 2) % CH] : nxt[(i + 2) % CH], o2);
                        double s = o.used ? 1.0 : 0.0;
                        if (!first && o.used) {
                            const double r = it_norm(o, dp[i]);
                            s = r > p.delta ? p.delta / r : 1.0;
                        }
                        rays::normal_eq g;
                        g.a00 = s * o.w[0];
                        g.a01 = s * o.w[1];
                        g.a02 = s * o.w[2];
                        g.a11 = s * o.w[3];
                        g.a12 = s * o.w[4];
                        g.a22 = s * o.w[5];
                        double a, bb, c, E[9], Di[6], q[3];
                        trj_band(t, T, p.lv, p.la, a, bb, c);
                        for (int u = 0; u < 3; ++u) g.rhs[u] = -(a * o.z[u] + bb * o1.z[u] + c * o2.z[u] + bp1 * zp1[u] + cp2 * zp2[u]);
                        ch.step(g, a, bb, c, E, Di, q);
                        const int64_t row = (int64_t)t * p.tracks;
                        for (int u = 0; u < 9; ++u) S[(IT_E + u) * plane + row] = E[u];
                        for (int u = 0; u < 6; ++u) S[(IT_DINV + u) * plane + row] = Di[u];
                        for (int u = 0; u < 3; ++u) S[(IT_Q + u) * plane + row] = q[u];
                        for (int u = 0; u < 3; ++u) {
                            zp2[u] = zp1[u];
                            zp1[u] = o.z[u];
                        }
                        cp2 = cp1;
                        cp1 = c;
                        bp1 = bb;
                        used_frames += o.used ? 1 : 0;
                        if (last) {
                            const int64_t at = base + (int64_t)t * J;
                            since = o.used ? 0 : (since < IT_FAR ? since + 1 : IT_FAR);
                            weight[at] = (float)s;
                            valid[at] = since <= p.max_gap ? 1 : 0;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    cur[i] = nxt[i];
                    nxt[i] = far[i];
                    for (int c = 0; c < 3; ++c) dp[i][c] = dn[i][c];
                }
            }
            if (first) {
                // solvable: (a) enough used frames for the penalty's null space, (b) no scalar pivot at or below the ratio of the largest
                // diagonal entry (include/egorear_hip.h; a NaN anywhere fails)
                const bool enough = p.lv > 0.0 ? used_frames >= 1 : (T >= 3 ? used_frames >= 2 : used_frames == T);
                if (!(enough && ch.finite && ch.min_pivot > p.min_pivot_ratio * ch.max_diag)) {
                    it_dead(p, base, k, pose, valid, residual, weight, energy);
                    return;
                }
            }
        }
        // ---- backward sweep: substitute; d_t goes to the q slots
        constexpr int CH = IT_CH_BWD;
        double x1[3] = {0.0, 0.0, 0.0}, x2[3] = {0.0, 0.0, 0.0};
        double cs[CH][IT_SOLVE_SLOTS], ns[CH][IT_SOLVE_SLOTS];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int64_t row = (int64_t)it_max(T - 1 - i, 0) * p.tracks;
            for (int s = 0; s < IT_SOLVE_SLOTS; ++s) cs[i][s] = S[s * plane + row];
        }
        for (int t1 = T - 1; t1 >= 0; t1 -= CH) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {                           // (rows below every row this chunk writes; past the start row 0, unused)
                const int64_t row = (int64_t)it_max(t1 - CH - i, 0) * p.tracks;
                for (int s = 0; s < IT_SOLVE_SLOTS; ++s) ns[i][s] = S[s * plane + row];
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int t = t1 - i;
                if (t >= 0) {
                    double a, bb, c, fx[3], x[3];
                    trj_band(t, T, p.lv, p.la, a, bb, c);
                    const double* E = cs[i] + IT_E;
                    rt_sym_vec(cs[i] + IT_DINV, x2, fx);
                    for (int r = 0; r < 3; ++r) x[r] = cs[i][IT_Q + r] - (E[r] * x1[0] + E[3 + r] * x1[1] + E[6 + r] * x1[2]) - c * fx[r];
                    const int64_t row = (int64_t)t * p.tracks;
                    for (int r = 0; r < 3; ++r) S[(IT_Q + r) * plane + row] = x[r];
                    for (int r = 0; r < 3; ++r) {
                        x2[r] = x1[r];
                        x1[r] = x[r];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < CH; ++i)
                for (int s = 0; s < IT_SOLVE_SLOTS; ++s) cs[i][s] = ns[i][s];
        }
    }
    // ---- output pass, from the last frame down: no chain - the pose z_t + d_t, the displacements, the energy, the other half of the validity
    double e_data = 0.0, e_vel = 0.0, e_acc = 0.0, x1[3] = {0.0, 0.0, 0.0}, x2[3] = {0.0, 0.0, 0.0};
    int until = IT_FAR;
#pragma unroll 2
    for (int t = T - 1; t >= 0; --t) {
        const int64_t row = (int64_t)t * p.tracks, at = base + (int64_t)t * J;
        it_raw raw;
        it_fetch(p, at, raw);
        it_frame o;
        it_decode(raw, o);
        const double d[3] = {S[IT_Q * plane + row], S[(IT_Q + 1) * plane + row], S[(IT_Q + 2) * plane + row]};
        const double x[3] = {o.z[0] + d[0], o.z[1] + d[1], o.z[2] + d[2]};
        for (int c = 0; c < 3; ++c) pose[at * 3 + c] = (float)x[c];
        const double r = o.used ? it_norm(o, d) : 0.0;
        e_data += p.delta > 0.0 && r > p.delta ? 2.0 * p.delta * r - p.delta * p.delta : r * r;
        residual[at] = (float)r;
        if (t < T - 1) {
            const double v0 = x1[0] - x[0], v1 = x1[1] - x[1], v2 = x1[2] - x[2];
            e_vel += v0 * v0 + v1 * v1 + v2 * v2;
        }
        if (t < T - 2) {
            const double a0 = x2[0] - 2.0 * x1[0] + x[0], a1 = x2[1] - 2.0 * x1[1] + x[1], a2 = x2[2] - 2.0 * x1[2] + x[2];
            e_acc += a0 * a0 + a1 * a1 + a2 * a2;
        }
        until = o.used ? 0 : (until < IT_FAR ? until + 1 : IT_FAR);
        if (until <= p.max_gap) valid[at] = 1;                       // (the forward sweep wrote the flag of the frames before t)
        for (int c = 0; c < 3; ++c) {
            x2[c] = x1[c];
            x1[c] = x[c];
        }
    }
    energy[k] = (float)(e_data + p.lv * e_vel + p.la * e_acc);
}

__global__ __launch_bounds__(128) void joint_info_kernel(const float* points, const float* conf, const float* cams, const float* ctm, int64_t cells,
                                                         int V, int J, float sx, float sy, float thr, float min_det_ratio, float* info,
                                                         uint8_t* views, float* sigma, uint8_t* valid) {
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= cells) return;
    ji_one(points, conf, cams, ctm, V, J, (double)sx, (double)sy, thr, (double)min_det_ratio, i, info, views, sigma, valid);
}

__global__ __launch_bounds__(64) void info_track_kernel(it_args p, double* ws, float* pose, uint8_t* valid, float* residual, float* weight,
                                                        float* energy) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= p.tracks) return;
    it_solve_one(p, k, ws, pose, valid, residual, weight, energy);
}

inline bool it_number(float v) { return v >= 0.0f && v <= 3.402823466e38f; }       // non-negative and finite

inline bool it_shape_ok(int32_t N, int32_t T, int32_t J) {
    return N >= 1 && J >= 1 && T >= 1 && T <= IT_MAX_T && (int64_t)N * T * J * 6 < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int egr_joint_info_f32(const float* points, const float* conf, const float* cams, const float* ctm, int32_t B, int32_t V, int32_t J,
                                  float sx, float sy, float threshold, float min_det_ratio, float* info, uint8_t* views, float* sigma,
                                  uint8_t* valid, void* stream) {
    if (!points || !conf || !cams || !info || !views || !sigma || !valid) return EGR_ENULL;
    if (!rays::shape_ok(B, V, J, sx, sy, min_det_ratio) || !(threshold == threshold)) return EGR_EINVAL;
    const int64_t cells = (int64_t)B * J;
    hipLaunchKernelGGL(joint_info_kernel, dim3((unsigned)((cells + 127) / 128)), dim3(128), 0, (hipStream_t)stream, points, conf, cams, ctm, cells,
                       V, J, sx, sy, threshold, min_det_ratio, info, views, sigma, valid);
    return egr_launch_status();
}

extern "C" int64_t egr_info_track_workspace_bytes(int32_t N, int32_t T, int32_t J) {
    if (!it_shape_ok(N, T, J)) return 0;
    return (int64_t)IT_SOLVE_SLOTS * T * N * J * (int64_t)sizeof(double);
}

extern "C" int egr_info_track_f32(const float* pose, const float* info, const uint8_t* obs, int32_t N, int32_t T, int32_t J, float vel_weight,
                                  float accel_weight, float huber, int32_t reweights, int32_t max_gap, double min_pivot_ratio, double* workspace,
                                  int64_t workspace_bytes, float* pose_out, uint8_t* valid, float* residual, float* weight, float* energy,
                                  void* stream) {
    if (!pose || !info || !workspace || !pose_out || !valid || !residual || !weight || !energy) return EGR_ENULL;
    if (!it_shape_ok(N, T, J)) return EGR_EINVAL;
    if (!it_number(vel_weight) || !it_number(accel_weight) || !(vel_weight > 0.0f || accel_weight > 0.0f)) return EGR_EINVAL;
    if (!it_number(huber) || reweights < 0 || reweights > IT_MAX_REWEIGHTS || (reweights > 0) != (huber > 0.0f) || max_gap < 0)
        return EGR_EINVAL;
    if (!(min_pivot_ratio >= 0.0 && min_pivot_ratio < 1.0)) return EGR_EINVAL;
    if (workspace_bytes < egr_info_track_workspace_bytes(N, T, J)) return EGR_EWORKSPACE;
    it_args p;
    p.pose = pose;
    p.info = info;
    p.obs = obs;
    p.T = T;
    p.J = J;
    p.tracks = (int64_t)N * J;
    p.lv = (double)vel_weight;
    p.la = (double)accel_weight;
    p.delta = (double)huber;
    p.min_pivot_ratio = min_pivot_ratio;
    p.reweights = reweights;
    p.max_gap = max_gap;
    hipLaunchKernelGGL(info_track_kernel, dim3((unsigned)((p.tracks + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p, workspace, pose_out, valid,
                       residual, weight, energy);
    return egr_launch_status();
}
