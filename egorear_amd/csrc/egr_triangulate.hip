// Fisheye triangulation of decoded 2-D joints into 3-D: forward and backward.
// The inverse of the projection of egr_fisheye.h (utils/camera_models.py:53-104): image point -> unit ray (the C2W polynomial seeds
// theta, Newton on the W2C polynomial the projection uses refines it), rays -> the point p of the device frame that minimises
// sum_v w_v |P_v (R_v p + t_v)|^2,  P = I - d d^T:   A p = b,  A = sum w R^T P R,  b = -sum w R^T P t.
// The camera record, the ray, the extrinsics and the normal equations are those of egr_rays.h.
//
// One thread owns one (frame, joint) and loops over the 2..4 views: no atomics, no LDS, no cross-lane traffic - a pair's bits depend
// on its own operands only.  The launch is 64 x 15 threads and latency-bound, so the arithmetic is done in fp64 throughout (inputs
// and outputs stay fp32): every output is the float64 statement's value to within an fp32 ulp, and the backward recomputes the forward
// from the operands instead of reading rounded fp32 intermediates back.  A pair's rays (the trigonometry) are computed once per view.
#include "egr_rays.h"

namespace {

struct tri_solution {
    rays::ray ray[rays::MAX_V];
    double p[3], cost, wsum, r[rays::MAX_V];
    rays::ldl f;
    bool ok;
};

// the forward of one (frame, joint): normal equations over the views, LDL^T, then the ray distances at the solution.
// (the view loops are unrolled over MAX_V so that the per-view arrays are registers, not scratch: 116 / 168 VGPRs, 19 / 24 KB of
// code.  A rolled loop that picks a view's slot by compare-and-select is folded back into an indexed - scratch - access by the compiler.)
__host__ __device__ inline void tri_solve(const float* coords, const float* conf, const float* cams, const float* ctm, int b, int j, int V,
                                          int J, double sx, double sy, float thr, double min_det_ratio, tri_solution& s) {
    rays::normal_eq n;
    double R[9], t[3];
    int used = 0;
    s.wsum = 0.0;
#pragma unroll
    for (int v = 0; v < rays::MAX_V; ++v) {
        s.r[v] = 0.0;
        s.ray[v].w = 0.0;
        if (v >= V) continue;
        rays::ray& ry = s.ray[v];
        rays::make_ray(coords, conf, cams + v * rays::REC, ((int64_t)b * V + v) * J + j, sx, sy, thr, ry);
        if (ry.w == 0.0) continue;
        rays::extrinsics(cams + v * rays::REC, ctm, (int64_t)b * V + v, R, t);
        ++used;
        s.wsum += ry.w;
        // rays::add_ray(R, t, ry.d, ry.w, n), written out.  As a call the compiler pairs the term's operations differently into its
        // two-wide fp64 forms: the backward measured 0.2 us slower and last bits of resid and g_conf moved where they are rounding
        // residue.  tests/test_gpu_consensus.py holds this kernel and the consensus, which calls add_ray, to each other.
        double e[3], rt[3];
        const double dt = ry.d[0] * t[0] + ry.d[1] * t[1] + ry.d[2] * t[2];
        for (int k = 0; k < 3; ++k) {
            e[k] = R[k] * ry.d[0] + R[3 + k] * ry.d[1] + R[6 + k] * ry.d[2];
            rt[k] = R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2];
        }
        n.a00 += ry.w * (rays::rr(R, 0, 0) - e[0] * e[0]);
        n.a01 += ry.w * (rays::rr(R, 0, 1) - e[0] * e[1]);
        n.a02 += ry.w * (rays::rr(R, 0, 2) - e[0] * e[2]);
        n.a11 += ry.w * (rays::rr(R, 1, 1) - e[1] * e[1]);
        n.a12 += ry.w * (rays::rr(R, 1, 2) - e[1] * e[2]);
        n.a22 += ry.w * (rays::rr(R, 2, 2) - e[2] * e[2]);
        for (int k = 0; k < 3; ++k) n.rhs[k] -= ry.w * (rt[k] - e[k] * dt);
    }
    s.ok = rays::factor(n, min_det_ratio, s.f) && used >= 2;
    s.p[0] = s.p[1] = s.p[2] = s.cost = 0.0;
    if (!s.ok) return;
    rays::ldl_solve(s.f, n.rhs, s.p);
    double acc = 0.0;
#pragma unroll
    for (int v = 0; v < rays::MAX_V; ++v) {
        const rays::ray& ry = s.ray[v];
        if (v >= V || ry.w == 0.0) continue;
        double q[3];
        rays::extrinsics(cams + v * rays::REC, ctm, (int64_t)b * V + v, R, t);
        rays::apply(R, t, s.p, q);
        const double dq = ry.d[0] * q[0] + ry.d[1] * q[1] + ry.d[2] * q[2];
        const double r0 = q[0] - ry.d[0] * dq, r1 = q[1] - ry.d[1] * dq, r2 = q[2] - ry.d[2] * dq;
        const double rr = r0 * r0 + r1 * r1 + r2 * r2;
        s.r[v] = sqrt(rr);
        acc += ry.w * rr;
    }
    s.cost = acc / s.wsum;
}

__host__ __device__ inline void tri_forward_one(const float* coords, const float* conf, const float* cams, const float* ctm, int idx, int V,
                                                int J, float sx, float sy, float thr, float min_det_ratio, float* pts, float* cost,
                                                float* resid, uint8_t* ok) {
    const int b = idx / J, j = idx - b * J;
    tri_solution s;
    tri_solve(coords, conf, cams, ctm, b, j, V, J, (double)sx, (double)sy, thr, (double)min_det_ratio, s);
    for (int k = 0; k < 3; ++k) pts[(int64_t)idx * 3 + k] = (float)s.p[k];
    cost[idx] = (float)s.cost;
    ok[idx] = s.ok ? 1 : 0;
#pragma unroll
    for (int v = 0; v < rays::MAX_V; ++v)
        if (v < V) resid[((int64_t)b * V + v) * J + j] = (float)s.r[v];
}

// L = g_pts . p + g_cost * cost.  Through the solve: dp = A^-1 (db - dA p), so with lambda = A^-1 g_pts and mu = R lambda
//   dL/dw = -mu . P q,   dL/dd = w ((d . q) mu + (mu . d) q);
// through the cost at fixed p (the envelope theorem: p minimises it):  dc/dw = (r^2 - c) / W,  dc/dd = -2 w (d . q) q / W;
// through the ray:  d = (ux cos, uy cos, -sin)(theta(rho)),  dtheta/drho = 1 / W2C'(theta).
__host__ __device__ inline void tri_backward_one(const float* coords, const float* conf, const float* cams, const float* ctm, int idx, int V,
                                                 int J, float sx, float sy, float thr, float min_det_ratio, const float* g_pts,
                                                 const float* g_cost, float* g_coords, float* g_conf) {
    const int b = idx / J, j = idx - b * J;
    tri_solution s;
    tri_solve(coords, conf, cams, ctm, b, j, V, J, (double)sx, (double)sy, thr, (double)min_det_ratio, s);
    double gp[3] = {0, 0, 0}, lam[3] = {0, 0, 0};
    const double gc = g_cost ? (double)g_cost[idx] : 0.0;
    if (g_pts)
        for (int k = 0; k < 3; ++k) gp[k] = (double)g_pts[(int64_t)idx * 3 + k];
    if (s.ok) rays::ldl_solve(s.f, gp, lam);
#pragma unroll
    for (int v = 0; v < rays::MAX_V; ++v) {
        if (v >= V) continue;
        const rays::ray& ry = s.ray[v];
        const int64_t at = ((int64_t)b * V + v) * J + j;
        double gx = 0.0, gy = 0.0, gw = 0.0;
        if (s.ok && ry.w != 0.0) {
            double R[9], t[3], q[3], mu[3], gd[3];
            rays::extrinsics(cams + v * rays::REC, ctm, (int64_t)b * V + v, R, t);
            rays::apply(R, t, s.p, q);
            for (int r = 0; r < 3; ++r) mu[r] = R[r * 3] * lam[0] + R[r * 3 + 1] * lam[1] + R[r * 3 + 2] * lam[2];
            const double dq = ry.d[0] * q[0] + ry.d[1] * q[1] + ry.d[2] * q[2];
            const double md = ry.d[0] * mu[0] + ry.d[1] * mu[1] + ry.d[2] * mu[2];
            const double mq = mu[0] * q[0] + mu[1] * q[1] + mu[2] * q[2];
            gw = -(mq - md * dq) + gc * (s.r[v] * s.r[v] - s.cost) / s.wsum;
            const double cq = md - 2.0 * gc * dq / s.wsum;
            for (int r = 0; r < 3; ++r) gd[r] = ry.w * (dq * mu[r] + cq * q[r]);
            if (!ry.axis) {
                const double g_theta = -(gd[0] * ry.ux + gd[1] * ry.uy) * ry.st - gd[2] * ry.ct;
                const double g_rho = g_theta / ry.dw2c;
                const double cross = (gd[0] * ry.uy - gd[1] * ry.ux) * ry.ct / ry.rho;     // (g_ux uy - g_uy ux) / rho
                const double g_dx = g_rho * ry.ux + ry.uy * cross, g_dy = g_rho * ry.uy - ry.ux * cross;
                gx = g_dx * (double)sx * (double)cams[v * rays::REC + 3];
                gy = g_dy * (double)sy * (double)cams[v * rays::REC + 4];
            }
        }
        g_coords[at * 2 + 0] = (float)gx;
        g_coords[at * 2 + 1] = (float)gy;
        g_conf[at] = (float)gw;
    }
}

__global__ __launch_bounds__(64) void triangulate_kernel(const float* coords, const float* conf, const float* cams, const float* ctm, int pairs,
                                                         int V, int J, float sx, float sy, float thr, float min_det_ratio, float* pts,
                                                         float* cost, float* resid, uint8_t* ok) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= pairs) return;
    tri_forward_one(coords, conf, cams, ctm, idx, V, J, sx, sy, thr, min_det_ratio, pts, cost, resid, ok);
}

__global__ __launch_bounds__(64) void triangulate_bwd_kernel(const float* coords, const float* conf, const float* cams, const float* ctm,
                                                             int pairs, int V, int J, float sx, float sy, float thr, float min_det_ratio,
                                                             const float* g_pts, const float* g_cost, float* g_coords, float* g_conf) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= pairs) return;
    tri_backward_one(coords, conf, cams, ctm, idx, V, J, sx, sy, thr, min_det_ratio, g_pts, g_cost, g_coords, g_conf);
}

inline bool tri_shape_ok(int32_t B, int32_t V, int32_t J, float sx, float sy, float thr, float min_det_ratio) {
    return rays::shape_ok(B, V, J, sx, sy, min_det_ratio) && thr == thr;
}

}  // namespace

extern "C" int egr_triangulate_f32(const float* coords, const float* conf, const float* cams, const float* ctm, int32_t B, int32_t V, int32_t J,
                                   float sx, float sy, float threshold, float min_det_ratio, float* pts, float* cost, float* resid,
                                   uint8_t* ok, void* stream) {
    if (!coords || !conf || !cams || !pts || !cost || !resid || !ok) return EGR_ENULL;
    if (!tri_shape_ok(B, V, J, sx, sy, threshold, min_det_ratio)) return EGR_EINVAL;
    const int pairs = B * J;
    hipLaunchKernelGGL(triangulate_kernel, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream, coords, conf, cams, ctm,
                       pairs, V, J, sx, sy, threshold, min_det_ratio, pts, cost, resid, ok);
    return egr_launch_status();
}

extern "C" int egr_triangulate_bwd_f32(const float* coords, const float* conf, const float* cams, const float* ctm, int32_t B, int32_t V,
                                       int32_t J, float sx, float sy, float threshold, float min_det_ratio, const float* g_pts,
                                       const float* g_cost, float* g_coords, float* g_conf, void* stream) {
    if (!coords || !conf || !cams || !g_coords || !g_conf) return EGR_ENULL;
    if (!tri_shape_ok(B, V, J, sx, sy, threshold, min_det_ratio)) return EGR_EINVAL;
    const int pairs = B * J;
    hipLaunchKernelGGL(triangulate_bwd_kernel, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream, coords, conf, cams, ctm,
                       pairs, V, J, sx, sy, threshold, min_det_ratio, g_pts, g_cost, g_coords, g_conf);
    return egr_launch_status();
}
