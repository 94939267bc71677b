// The ray record of camera.packed_rays() and the math every 3-D decoder builds on it: the record's layout,
// the extrinsics, image point -> unit ray, and the weighted normal equations of the rays' least-squares intersection.  The one
// device-side statement of all four: egr_triangulate.hip, egr_consensus.hip and egr_volume.hip include it, nothing restates it.
#pragma once
#include "egr_common.h"
#include "egr_fisheye.h"
#include <math.h>

namespace rays {

// [npoly, cx, cy, W, H, W2C[12] | nc2w, C2W[8] | flip, off_x, off_y, off_z]: the first 17 floats are the record of
// camera.packed(), egrf::CAM_REC, which this one extends - the projection of egr_fisheye.h reads a ray record as it is.
constexpr int REC = 30;
constexpr int W2C = 5, MAX_W2C = 12, NC2W = 17, C2W = 18, MAX_C2W = 8, FLIP = 26, OFF = 27;
static_assert(W2C + MAX_W2C == egrf::CAM_REC && C2W + MAX_C2W == FLIP && OFF + 3 == REC, "the ray record extends the camera record");
constexpr int MAX_V = 4;      // 2 to 4 views
// the C2W seed is within 2.5e-5 rad of the root and W2C' >= 275: one step leaves 1e-11 rad (below half an fp32 ulp of theta), the
// second 4e-16 - a third changes nothing even in fp64 (tests/test_triangulate_host.py measures all three)
constexpr int NEWTON = 2;
constexpr double RHO_GUARD = 1e-4;     // pixels: closer to the image centre the ray is the optical axis

// the number of W2C coefficients a record may claim
__host__ __device__ inline int w2c_degree(const float* cam) {
    const int nw = (int)cam[0];
    return nw < 0 ? 0 : (nw > MAX_W2C ? MAX_W2C : nw);
}

// what the entries of the triangulation and of the consensus ask of their common arguments
inline bool shape_ok(int32_t B, int32_t V, int32_t J, float sx, float sy, float min_det_ratio) {
    return B > 0 && J > 0 && V >= 2 && V <= MAX_V && (int64_t)B * J * V < (1 << 30) && sx > 0.f && sx <= 3.0e38f && sy > 0.f &&
           sy <= 3.0e38f && min_det_ratio >= 0.f && min_det_ratio <= 3.0e38f;
}

struct ray {
    double w;                  // 0: the view is excluded
    double d[3];               // unit ray, camera frame
    double ux, uy, rho, st, ct, dw2c;
    bool axis;
};

// image point -> ray of view v of pair (b, j): the trigonometry of a pair is done once per view and kept in registers
__host__ __device__ inline void make_ray(const float* coords, const float* conf, const float* cam, int64_t at, double sx, double sy,
                                         float thr, ray& o) {
    const float xf = coords[at * 2 + 0], yf = coords[at * 2 + 1], cf = conf[at];
    const bool use = cf >= thr && cf > 0.f && isfinite(cf) && isfinite(xf) && isfinite(yf);
    o.w = use ? (double)cf : 0.0;
    const double x = use ? (double)xf : 0.0, y = use ? (double)yf : 0.0;
    const double cx = cam[1], cy = cam[2], W = cam[3], H = cam[4];
    const double dx = x * sx * W - cx, dy = y * sy * H - cy;
    const double rho = sqrt(dx * dx + dy * dy);        // (pixels: no scaling against overflow is needed)
    o.axis = !(rho >= RHO_GUARD);
    o.rho = o.axis ? 1.0 : rho;
    const double inv_rho = 1.0 / o.rho;                // one division serves the unit vector and the seed
    o.ux = o.axis ? 0.0 : dx * inv_rho;
    o.uy = o.axis ? 0.0 : dy * inv_rho;
    const int nw = w2c_degree(cam);
    int nc = (int)cam[NC2W];
    nc = nc < 0 ? 0 : (nc > MAX_C2W ? MAX_C2W : nc);
    double f = 0.0;
    for (int i = nc - 1; i >= 0; --i) f = f * o.rho + (double)cam[C2W + i];
    double theta = atan(f * inv_rho), dp = 0.0;
    for (int it = 0; it <= NEWTON; ++it) {              // the last pass only evaluates W2C' at the final theta
        double p = 0.0;
        dp = 0.0;
        for (int i = nw - 1; i >= 0; --i) {
            dp = dp * theta + p;
            p = p * theta + (double)cam[W2C + i];
        }
        if (it < NEWTON) theta -= (p - o.rho) / dp;
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
__host__ __device__ inline void extrinsics(const float* cam, const float* ctm, int64_t bv, double* R, double* t) {
    if (ctm) {           // rw: p_cam = (M . [p * 0.01, 1]) * 100 = M3 p + 100 m_t
        const float* m = ctm + bv * 16;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)m[r * 4 + c];
            t[r] = 100.0 * (double)m[r * 4 + 3];
        }
    } else {             // syn: this camera alone, un-chained - the back cameras flip x and y, then the offset
        const double fl = cam[FLIP] != 0.f ? -1.0 : 1.0;
        for (int i = 0; i < 9; ++i) R[i] = 0.0;
        R[0] = fl;
        R[4] = fl;
        R[8] = 1.0;
        for (int r = 0; r < 3; ++r) t[r] = (double)cam[OFF + r];
    }
}

__host__ __device__ inline void apply(const double* R, const double* t, const double* p, double* q) {
    for (int r = 0; r < 3; ++r) q[r] = R[r * 3] * p[0] + R[r * 3 + 1] * p[1] + R[r * 3 + 2] * p[2] + t[r];
}

// the point p that minimises  sum_v w_v |P_v (R_v p + t_v)|^2,  P = I - d d^T:   A p = b,  A = sum w R^T P R,  b = -sum w R^T P t
struct normal_eq {
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, rhs[3] = {0, 0, 0};
};

struct ldl {      // A = L D L^T
    double d1, d2, d3, l21, l31, l32;
};

__host__ __device__ inline double rr(const double* R, int k, int l) { return R[k] * R[l] + R[3 + k] * R[3 + l] + R[6 + k] * R[6 + l]; }

// one view's term: G = R^T P R = R^T R - e e^T with e = R^T d;  h = R^T P t = R^T t - e (d . t)
// (tri_solve of egr_triangulate.hip writes these lines out in its unrolled loop and says why: a change here is a change there)
__host__ __device__ inline void add_ray(const double* R, const double* t, const double* d, double w, normal_eq& n) {
    double e[3], rt[3];
    const double dt = d[0] * t[0] + d[1] * t[1] + d[2] * t[2];
    for (int k = 0; k < 3; ++k) {
        e[k] = R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2];
        rt[k] = R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2];
    }
    n.a00 += w * (rr(R, 0, 0) - e[0] * e[0]);
    n.a01 += w * (rr(R, 0, 1) - e[0] * e[1]);
    n.a02 += w * (rr(R, 0, 2) - e[0] * e[2]);
    n.a11 += w * (rr(R, 1, 1) - e[1] * e[1]);
    n.a12 += w * (rr(R, 1, 2) - e[1] * e[2]);
    n.a22 += w * (rr(R, 2, 2) - e[2] * e[2]);
    for (int k = 0; k < 3; ++k) n.rhs[k] -= w * (rt[k] - e[k] * dt);
}

// false: the rays do not fix a point - A is not positive definite, or too flat for its size (a NaN anywhere fails the comparisons:
// such a system is reported as not solvable, never as numbers)
__host__ __device__ inline bool factor(const normal_eq& n, double min_det_ratio, ldl& f) {
    f.d1 = n.a00;
    f.l21 = n.a01 / f.d1;
    f.l31 = n.a02 / f.d1;
    f.d2 = n.a11 - f.l21 * n.a01;
    f.l32 = (n.a12 - f.l31 * n.a01) / f.d2;
    f.d3 = n.a22 - f.l31 * n.a02 - f.l32 * f.l32 * f.d2;
    const double det = f.d1 * f.d2 * f.d3, tr3 = (n.a00 + n.a11 + n.a22) / 3.0;
    return f.d1 > 0.0 && f.d2 > 0.0 && f.d3 > 0.0 && det > min_det_ratio * tr3 * tr3 * tr3;
}

__host__ __device__ inline void ldl_solve(const ldl& f, const double* rhs, double* x) {
    const double y1 = rhs[0], y2 = rhs[1] - f.l21 * y1, y3 = rhs[2] - f.l31 * y1 - f.l32 * y2;
    x[2] = y3 / f.d3;
    x[1] = y2 / f.d2 - f.l32 * x[2];
    x[0] = y1 / f.d1 - f.l21 * x[1] - f.l31 * x[2];
}

}  // namespace rays
