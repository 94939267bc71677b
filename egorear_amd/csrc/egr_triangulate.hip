// Fisheye triangulation of decoded 2-D joints into 3-D: forward and backward.
// The inverse of the projection of egr_fisheye.h (utils/camera_models.py:53-104): image point -> unit ray (the C2W polynomial seeds
// theta, Newton on the W2C polynomial the projection uses refines it), rays -> the point p of the device frame that minimises
// sum_v w_v |P_v (R_v p + t_v)|^2,  P = I - d d^T:   A p = b,  A = sum w R^T P R,  b = -sum w R^T P t.
//
// One thread owns one (frame, joint) and loops over the 2..4 views: no atomics, no LDS, no cross-lane traffic - a pair's bits depend
// on its own operands only.  The launch is 64 x 15 threads and latency-bound, so the arithmetic is done in fp64 throughout (inputs
// and outputs stay fp32): every output is the float64 statement's value to within an fp32 ulp, and the backward recomputes the forward
// from the operands instead of reading rounded fp32 intermediates back.  A pair's rays (the trigonometry) are computed once per view.
#include "egr_common.h"
#include <math.h>

namespace {

// camera record of camera.packed_rays(): [npoly, cx, cy, W, H, W2C[12] | nc2w, C2W[8] | flip, off_x, off_y, off_z]
constexpr int TRI_REC = 30;
constexpr int TRI_W2C = 5, TRI_MAX_W2C = 12, TRI_NC2W = 17, TRI_C2W = 18, TRI_MAX_C2W = 8, TRI_FLIP = 26, TRI_OFF = 27;
constexpr int TRI_MAX_V = 4;
// the C2W seed is within 2.5e-5 rad of the root and W2C' >= 275: one step leaves 1e-11 rad (below half an fp32 ulp of theta), the
// second 4e-16 - a third changes nothing even in fp64 (tests/test_triangulate_host.py measures all three)
constexpr int TRI_NEWTON = 2;
constexpr double TRI_RHO_GUARD = 1e-4;     // pixels: closer to the image centre the ray is the optical axis

struct tri_ray {
    double w;                  // 0: the view is excluded
    double d[3];               // unit ray, camera frame
    double ux, uy, rho, st, ct, dw2c;
    bool axis;
};

// image point -> ray of view v of pair (b, j): the trigonometry of a pair is done once per view and kept in registers
__host__ __device__ inline void tri_make_ray(const float* coords, const float* conf, const float* cam, int64_t at, double sx, double sy,
                                             float thr, tri_ray& o) {
    const float xf = coords[at * 2 + 0], yf = coords[at * 2 + 1], cf = conf[at];
    const bool use = cf >= thr && cf > 0.f && isfinite(cf) && isfinite(xf) && isfinite(yf);
    o.w = use ? (double)cf : 0.0;
    const double x = use ? (double)xf : 0.0, y = use ? (double)yf : 0.0;
    const double cx = cam[1], cy = cam[2], W = cam[3], H = cam[4];
    const double dx = x * sx * W - cx, dy = y * sy * H - cy;
    const double rho = sqrt(dx * dx + dy * dy);        // (pixels: no scaling against overflow is needed)
    o.axis = !(rho >= TRI_RHO_GUARD);
    o.rho = o.axis ? 1.0 : rho;
    const double inv_rho = 1.0 / o.rho;                // one division serves the unit vector and the seed
    o.ux = o.axis ? 0.0 : dx * inv_rho;
    o.uy = o.axis ? 0.0 : dy * inv_rho;
    int nw = (int)cam[0], nc = (int)cam[TRI_NC2W];
    nw = nw < 0 ? 0 : (nw > TRI_MAX_W2C ? TRI_MAX_W2C : nw);
    nc = nc < 0 ? 0 : (nc > TRI_MAX_C2W ? TRI_MAX_C2W : nc);
    double f = 0.0;
    for (int i = nc - 1; i >= 0; --i) f = f * o.rho + (double)cam[TRI_C2W + i];
    double theta = atan(f * inv_rho), dp = 0.0;
    for (int it = 0; it <= TRI_NEWTON; ++it) {          // the last pass only evaluates W2C' at the final theta
        double p = 0.0;
        dp = 0.0;
        for (int i = nw - 1; i >= 0; --i) {
            dp = dp * theta + p;
            p = p * theta + (double)cam[TRI_W2C + i];
        }
        if (it < TRI_NEWTON) theta -= (p - o.rho) / dp;
    }
    o.dw2c = dp;
    double st, ct;
    sincos(theta, &st, &ct);
    o.st = o.axis ? -1.0 : st;
    o.ct = o.axis ? 0.0 : ct;
    o.d[0] = o.ux * o.ct;
    o.d[1] = o.uy * o.ct;
    o.d[2] = -o.st;
}

// p_cam = R p + t in cm (a few loads: read again wherever it is needed rather than kept)
__host__ __device__ inline void tri_extrinsics(const float* cam, const float* ctm, int64_t bv, double* R, double* t) {
    if (ctm) {           // rw: p_cam = (M . [p * 0.01, 1]) * 100 = M3 p + 100 m_t
        const float* m = ctm + bv * 16;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)m[r * 4 + c];
            t[r] = 100.0 * (double)m[r * 4 + 3];
        }
    } else {             // syn: this camera alone, un-chained - the back cameras flip x and y, then the offset
        const double fl = cam[TRI_FLIP] != 0.f ? -1.0 : 1.0;
        for (int i = 0; i < 9; ++i) R[i] = 0.0;
        R[0] = fl;
        R[4] = fl;
        R[8] = 1.0;
        for (int r = 0; r < 3; ++r) t[r] = (double)cam[TRI_OFF + r];
    }
}

struct tri_solution {
    tri_ray ray[TRI_MAX_V];
    double p[3], cost, wsum, r[TRI_MAX_V];
    double d1, d2, d3, l21, l31, l32;      // A = L D L^T
    bool ok;
};

__host__ __device__ inline void tri_ldl_solve(const tri_solution& s, const double* rhs, double* x) {
    const double y1 = rhs[0], y2 = rhs[1] - s.l21 * y1, y3 = rhs[2] - s.l31 * y1 - s.l32 * y2;
    x[2] = y3 / s.d3;
    x[1] = y2 / s.d2 - s.l32 * x[2];
    x[0] = y1 / s.d1 - s.l21 * x[1] - s.l31 * x[2];
}

__host__ __device__ inline void tri_apply(const double* R, const double* t, const double* p, double* q) {
    for (int r = 0; r < 3; ++r) q[r] = R[r * 3] * p[0] + R[r * 3 + 1] * p[1] + R[r * 3 + 2] * p[2] + t[r];
}

// the forward of one (frame, joint): normal equations over the views, LDL^T, then the ray distances at the solution.
// (the view loops are unrolled over TRI_MAX_V so that the per-view arrays are registers, not scratch: 116 / 168 VGPRs, 19 / 24 KB of
// code.  A rolled loop that picks a view's slot by compare-and-select is folded back into an indexed - scratch - access by the compiler.)
__host__ __device__ inline void tri_solve(const float* coords, const float* conf, const float* cams, const float* ctm, int b, int j, int V,
                                          int J, double sx, double sy, float thr, double min_det_ratio, tri_solution& s) {
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, rhs[3] = {0, 0, 0};
    double R[9], t[3];
    int used = 0;
    s.wsum = 0.0;
#pragma unroll
    for (int v = 0; v < TRI_MAX_V; ++v) {
        s.r[v] = 0.0;
        s.ray[v].w = 0.0;
        if (v >= V) continue;
        tri_ray& ry = s.ray[v];
        tri_make_ray(coords, conf, cams + v * TRI_REC, ((int64_t)b * V + v) * J + j, sx, sy, thr, ry);
        if (ry.w == 0.0) continue;
        tri_extrinsics(cams + v * TRI_REC, ctm, (int64_t)b * V + v, R, t);
        ++used;
        s.wsum += ry.w;
        // G = R^T P R = R^T R - e e^T with e = R^T d;  h = R^T P t = R^T t - e (d . t)
        double e[3], rt[3];
        const double dt = ry.d[0] * t[0] + ry.d[1] * t[1] + ry.d[2] * t[2];
        for (int k = 0; k < 3; ++k) {
            e[k] = R[k] * ry.d[0] + R[3 + k] * ry.d[1] + R[6 + k] * ry.d[2];
            rt[k] = R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2];
        }
#define TRI_RR(k, l) (R[k] * R[l] + R[3 + k] * R[3 + l] + R[6 + k] * R[6 + l])
        a00 += ry.w * (TRI_RR(0, 0) - e[0] * e[0]);
        a01 += ry.w * (TRI_RR(0, 1) - e[0] * e[1]);
        a02 += ry.w * (TRI_RR(0, 2) - e[0] * e[2]);
        a11 += ry.w * (TRI_RR(1, 1) - e[1] * e[1]);
        a12 += ry.w * (TRI_RR(1, 2) - e[1] * e[2]);
        a22 += ry.w * (TRI_RR(2, 2) - e[2] * e[2]);
#undef TRI_RR
        for (int k = 0; k < 3; ++k) rhs[k] -= ry.w * (rt[k] - e[k] * dt);
    }
    s.d1 = a00;
    s.l21 = a01 / s.d1;
    s.l31 = a02 / s.d1;
    s.d2 = a11 - s.l21 * a01;
    s.l32 = (a12 - s.l31 * a01) / s.d2;
    s.d3 = a22 - s.l31 * a02 - s.l32 * s.l32 * s.d2;
    const double det = s.d1 * s.d2 * s.d3, tr3 = (a00 + a11 + a22) / 3.0;
    // (a NaN anywhere fails the comparisons: such a pair is reported as not ok, never as numbers)
    s.ok = used >= 2 && s.d1 > 0.0 && s.d2 > 0.0 && s.d3 > 0.0 && det > min_det_ratio * tr3 * tr3 * tr3;
    s.p[0] = s.p[1] = s.p[2] = s.cost = 0.0;
    if (!s.ok) return;
    tri_ldl_solve(s, rhs, s.p);
    double acc = 0.0;
#pragma unroll
    for (int v = 0; v < TRI_MAX_V; ++v) {
        const tri_ray& ry = s.ray[v];
        if (v >= V || ry.w == 0.0) continue;
        double q[3];
        tri_extrinsics(cams + v * TRI_REC, ctm, (int64_t)b * V + v, R, t);
        tri_apply(R, t, s.p, q);
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
    for (int v = 0; v < TRI_MAX_V; ++v)
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
    if (s.ok) tri_ldl_solve(s, gp, lam);
#pragma unroll
    for (int v = 0; v < TRI_MAX_V; ++v) {
        if (v >= V) continue;
        const tri_ray& ry = s.ray[v];
        const int64_t at = ((int64_t)b * V + v) * J + j;
        double gx = 0.0, gy = 0.0, gw = 0.0;
        if (s.ok && ry.w != 0.0) {
            double R[9], t[3], q[3], mu[3], gd[3];
            tri_extrinsics(cams + v * TRI_REC, ctm, (int64_t)b * V + v, R, t);
            tri_apply(R, t, s.p, q);
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
                gx = g_dx * (double)sx * (double)cams[v * TRI_REC + 3];
                gy = g_dy * (double)sy * (double)cams[v * TRI_REC + 4];
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
    return B > 0 && J > 0 && V >= 2 && V <= TRI_MAX_V && (int64_t)B * J * V < (1 << 30) && sx > 0.f && sx <= 3.0e38f && sy > 0.f &&
           sy <= 3.0e38f && thr == thr && min_det_ratio >= 0.f && min_det_ratio <= 3.0e38f;
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

// ------------------------------------------------------------------ consensus over candidate peaks
// Every view brings up to K candidate image points per joint (egr_peaks_f32); a hypothesis is one candidate from each of two views,
// h = (pair(a, b) * K + ka) * K + kb with the pairs in lexicographic order.  Its point is the two-ray least-squares intersection above
// (weights: the two scores, the same `ok`), projected into every view with the unclamped fisheye_pixel; a view supports it with
// its best  score * max(0, 1 - e^2 / tau^2),  e the distance (coords units) between the projection and the candidate.  The winner is
// the largest sum of the views' support among hypotheses that at least `min_views` views support, ties to the smaller h.
//
// One wave per (frame, joint), lanes = hypotheses (6 K^2 <= 96: two passes at K = 4).  The first V * K lanes build the candidates'
// rays once - the trigonometry - and park them in LDS, V more lanes the extrinsics; every lane then solves its pair and projects into
// the V views; one fixed-order butterfly (larger score, ties to the smaller h) picks the winner, whose lane writes the outputs.  fp64
// throughout, as above: a score's rounding decides a selection.  No atomics, a pair's bits depend on its own operands only.
#include "egr_fisheye.h"

namespace {

constexpr int CON_MAX_K = 4;
constexpr int CON_NONE = 0x7fffffff;

struct con_cand {
    double d[3];     // unit ray, camera frame
    double w;        // the score; 0: the candidate does not exist
    double x, y;     // coords units
};

__device__ __forceinline__ void con_add_ray(const double* R, const double* t, const con_cand& c, double& a00, double& a01, double& a02,
                                            double& a11, double& a12, double& a22, double* rhs) {
    // tri_solve's accumulation of one view: G = R^T R - e e^T with e = R^T d;  h = R^T t - e (d . t)
    double e[3], rt[3];
    const double dt = c.d[0] * t[0] + c.d[1] * t[1] + c.d[2] * t[2];
    for (int k = 0; k < 3; ++k) {
        e[k] = R[k] * c.d[0] + R[3 + k] * c.d[1] + R[6 + k] * c.d[2];
        rt[k] = R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2];
    }
#define CON_RR(k, l) (R[k] * R[l] + R[3 + k] * R[3 + l] + R[6 + k] * R[6 + l])
    a00 += c.w * (CON_RR(0, 0) - e[0] * e[0]);
    a01 += c.w * (CON_RR(0, 1) - e[0] * e[1]);
    a02 += c.w * (CON_RR(0, 2) - e[0] * e[2]);
    a11 += c.w * (CON_RR(1, 1) - e[1] * e[1]);
    a12 += c.w * (CON_RR(1, 2) - e[1] * e[2]);
    a22 += c.w * (CON_RR(2, 2) - e[2] * e[2]);
#undef CON_RR
    for (int k = 0; k < 3; ++k) rhs[k] -= c.w * (rt[k] - e[k] * dt);
}

__global__ __launch_bounds__(64) void consensus_kernel(const float* cand, const float* cscore, const int32_t* cindex, const float* cams,
                                                       const float* ctm, int V, int J, int K, float sx, float sy, float tau, int min_views,
                                                       float min_det_ratio, int32_t* choice, float* sel_coords, float* sel_conf,
                                                       float* score, int32_t* inliers, int32_t* hyp) {
    __shared__ con_cand s_c[TRI_MAX_V * CON_MAX_K];
    __shared__ double s_R[TRI_MAX_V][9], s_t[TRI_MAX_V][3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int b = pair / J, j = pair - b * J;
    if (lane < V * K) {
        const int v = lane / K, k = lane - v * K;
        const int64_t at = (((int64_t)b * V + v) * J + j) * K + k;
        tri_ray ry;
        // (threshold 0: the score must be positive and finite, the coordinates finite - tri_make_ray's own test)
        tri_make_ray(cand, cscore, cams + v * TRI_REC, at, (double)sx, (double)sy, 0.f, ry);
        const bool exists = cindex[at] >= 0 && ry.w != 0.0;
        con_cand c;
        c.w = exists ? ry.w : 0.0;
        c.d[0] = ry.d[0];
        c.d[1] = ry.d[1];
        c.d[2] = ry.d[2];
        c.x = exists ? (double)cand[at * 2 + 0] : 0.0;
        c.y = exists ? (double)cand[at * 2 + 1] : 0.0;
        s_c[lane] = c;
    } else if (lane >= 32 && lane < 32 + V) {
        const int v = lane - 32;
        double R[9], t[3];
        tri_extrinsics(cams + v * TRI_REC, ctm, (int64_t)b * V + v, R, t);
        for (int i = 0; i < 9; ++i) s_R[v][i] = R[i];
        for (int i = 0; i < 3; ++i) s_t[v][i] = t[i];
    }
    __syncthreads();

    const int kk = K * K, nhyp = (V * (V - 1) / 2) * kk;
    const double tau2 = (double)tau * (double)tau;
    double my = -1.0;             // a hypothesis that qualifies scores > 0
    int myh = CON_NONE, mypack = 0, myinl = 0;
    for (int h = lane; h < nhyp; h += 64) {
        const int pi = h / kk, rem = h - pi * kk, ka = rem / K, kb = rem - ka * K;
        int va = 0, left = pi;
        for (int n = V - 1; n > 1 && left >= n; --n) { left -= n; ++va; }
        const int vb = va + 1 + left;
        const con_cand ca = s_c[va * K + ka], cb = s_c[vb * K + kb];
        if (ca.w == 0.0 || cb.w == 0.0) continue;
        double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, rhs[3] = {0, 0, 0};
        con_add_ray(s_R[va], s_t[va], ca, a00, a01, a02, a11, a12, a22, rhs);
        con_add_ray(s_R[vb], s_t[vb], cb, a00, a01, a02, a11, a12, a22, rhs);
        tri_solution s;
        s.d1 = a00;
        s.l21 = a01 / s.d1;
        s.l31 = a02 / s.d1;
        s.d2 = a11 - s.l21 * a01;
        s.l32 = (a12 - s.l31 * a01) / s.d2;
        s.d3 = a22 - s.l31 * a02 - s.l32 * s.l32 * s.d2;
        const double det = s.d1 * s.d2 * s.d3, tr3 = (a00 + a11 + a22) / 3.0;
        if (!(s.d1 > 0.0 && s.d2 > 0.0 && s.d3 > 0.0 && det > (double)min_det_ratio * tr3 * tr3 * tr3)) continue;
        double p[3];
        tri_ldl_solve(s, rhs, p);
        double total = 0.0;
        int inl = 0, pack = 0;
        for (int v = 0; v < V; ++v) {
            const float* cam = cams + v * TRI_REC;
            double q[3];
            tri_apply(s_R[v], s_t[v], p, q);
            int nw = (int)cam[0];
            nw = nw < 0 ? 0 : (nw > TRI_MAX_W2C ? TRI_MAX_W2C : nw);
            double px, py;
            if (!egrf::fisheye_pixel<double, float>(cam + TRI_W2C, nw, (double)cam[1], (double)cam[2], q[0], q[1], q[2], &px, &py)) continue;
            const double u = px / ((double)sx * (double)cam[3]), w = py / ((double)sy * (double)cam[4]);
            double best = 0.0;
            int bk = -1;
            for (int k = 0; k < K; ++k) {
                const con_cand& c = s_c[v * K + k];
                if (c.w == 0.0) continue;
                const double dx = u - c.x, dy = w - c.y;
                const double keep = 1.0 - (dx * dx + dy * dy) / tau2;
                const double term = keep > 0.0 ? c.w * keep : 0.0;      // (NaN fails the comparison)
                if (term > best) { best = term; bk = k; }
            }
            if (bk >= 0) {
                total += best;
                ++inl;
                pack |= (bk + 1) << (4 * v);
            }
        }
        if (inl >= min_views && total > my) {     // (the lane's own hypotheses come in increasing h: '>' keeps the first)
            my = total;
            myh = h;
            mypack = pack;
            myinl = inl;
        }
    }
    double ws = my;
    int wh = myh;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(ws, o, 64);
        const int oh = __shfl_xor(wh, o, 64);
        if (os > ws || (os == ws && oh < wh)) { ws = os; wh = oh; }
    }
    const bool none = wh == CON_NONE;
    if (none ? lane == 0 : myh == wh) {
        for (int v = 0; v < V; ++v) {
            const int k = none ? -1 : ((mypack >> (4 * v)) & 7) - 1;
            const int64_t o = ((int64_t)b * V + v) * J + j;
            choice[o] = k;
            sel_coords[o * 2 + 0] = k >= 0 ? cand[(o * K + k) * 2 + 0] : 0.f;
            sel_coords[o * 2 + 1] = k >= 0 ? cand[(o * K + k) * 2 + 1] : 0.f;
            sel_conf[o] = k >= 0 ? cscore[o * K + k] : 0.f;
        }
        score[pair] = none ? 0.f : (float)ws;
        inliers[pair] = none ? 0 : myinl;
        hyp[pair] = none ? -1 : wh;
    }
}

}  // namespace

extern "C" int egr_consensus_f32(const float* cand, const float* cscore, const int32_t* cindex, const float* cams, const float* ctm, int32_t B,
                                 int32_t V, int32_t J, int32_t K, float sx, float sy, float max_reproj, int32_t min_views,
                                 float min_det_ratio, int32_t* choice, float* sel_coords, float* sel_conf, float* score, int32_t* inliers,
                                 int32_t* hyp, void* stream) {
    if (!cand || !cscore || !cindex || !cams || !choice || !sel_coords || !sel_conf || !score || !inliers || !hyp) return EGR_ENULL;
    if (!tri_shape_ok(B, V, J, sx, sy, 0.f, min_det_ratio) || K < 1 || K > CON_MAX_K || (int64_t)B * J * V * K >= (1 << 30) ||
        !(max_reproj > 0.f && max_reproj <= 3.0e38f) || min_views < 2 || min_views > V)
        return EGR_EINVAL;
    hipLaunchKernelGGL(consensus_kernel, dim3((unsigned)(B * J)), dim3(64), 0, (hipStream_t)stream, cand, cscore, cindex, cams, ctm, V, J, K,
                       sx, sy, max_reproj, min_views, min_det_ratio, choice, sel_coords, sel_conf, score, inliers, hyp);
    return egr_launch_status();
}
