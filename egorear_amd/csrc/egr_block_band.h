// The block-pentadiagonal elimination of the clip decoders with 3 x 3 blocks, written once: egr_raytrack.hip forms a
// frame's block (G_t, g_t) from the views' rays, egr_infotrack.hip from the frame's information matrix; both eliminate
//   (blockdiag(G_t) + (lv D1^T D1 + la D2^T D2) (x) I_3) x = (g_t)
// with rt_chain::step, one frame a call.
#pragma once
#include "egr_rays.h"

// ---- 3 x 3 helpers: a symmetric matrix is (00, 01, 02, 11, 12, 22), a general one row-major
__host__ __device__ inline void rt_sym_vec(const double* s, const double* x, double* y) {
    y[0] = s[0] * x[0] + s[1] * x[1] + s[2] * x[2];
    y[1] = s[1] * x[0] + s[3] * x[1] + s[4] * x[2];
    y[2] = s[2] * x[0] + s[4] * x[1] + s[5] * x[2];
}

// The elimination's carried state.
struct rt_chain {
    double Di1[6], Di2[6], M1[9], E1[9], y1[3], y2[3], c1 = 0.0, c2 = 0.0;
    double min_pivot = 1.7e308, max_diag = 0.0;
    bool finite = true;
    __host__ __device__ inline rt_chain() {
        for (int i = 0; i < 6; ++i) Di1[i] = Di2[i] = 0.0;
        for (int i = 0; i < 9; ++i) M1[i] = E1[i] = 0.0;
        for (int i = 0; i < 3; ++i) y1[i] = y2[i] = 0.0;
    }
    // pivot t: n = (G_t, g_t), (a, b, c) = trj_band -> E (9), Di (6), q (3)
    __host__ __device__ inline void step(const rays::normal_eq& n, double a, double b, double c, double* E, double* Di, double* q) {
        // D = G + a I - E1 M1^T - c2^2 Di2   (E1 M1^T = M1 Di1 M1^T is symmetric: its upper triangle)
        rays::normal_eq D;
        const double cc = c2 * c2;
#define RT_EM(i, j) (E1[i * 3] * M1[j * 3] + E1[i * 3 + 1] * M1[j * 3 + 1] + E1[i * 3 + 2] * M1[j * 3 + 2])
        D.a00 = n.a00 + a - RT_EM(0, 0) - cc * Di2[0];
        D.a01 = n.a01 - RT_EM(0, 1) - cc * Di2[1];
        D.a02 = n.a02 - RT_EM(0, 2) - cc * Di2[2];
        D.a11 = n.a11 + a - RT_EM(1, 1) - cc * Di2[3];
        D.a12 = n.a12 - RT_EM(1, 2) - cc * Di2[4];
        D.a22 = n.a22 + a - RT_EM(2, 2) - cc * Di2[5];
#undef RT_EM
        max_diag = fmax(max_diag, fmax(n.a00, fmax(n.a11, n.a22)) + a);
        rays::ldl f;
        rays::factor(D, 0.0, f);
        const double low = fmin(f.d1, fmin(f.d2, f.d3));
        finite = finite && f.d1 == f.d1 && f.d2 == f.d2 && f.d3 == f.d3;         // (fmin drops a NaN: it is kept here)
        min_pivot = fmin(min_pivot, low);
        // D^-1, a column at a time
        const double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
        double k0[3], k1[3], k2[3];
        rays::ldl_solve(f, e0, k0);
        rays::ldl_solve(f, e1, k1);
        rays::ldl_solve(f, e2, k2);
        Di[0] = k0[0];
        Di[1] = k1[0];
        Di[2] = k2[0];
        Di[3] = k1[1];
        Di[4] = k2[1];
        Di[5] = k2[2];
        // M = b I - c1 E1^T,  E = M D^-1
        double M[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) M[i * 3 + j] = (i == j ? b : 0.0) - c1 * E1[j * 3 + i];
        for (int i = 0; i < 3; ++i) rt_sym_vec(Di, M + i * 3, E + i * 3);           // row i of M D^-1 = D^-1 (row i of M)^T
        // y = g - E1 y1 - c2 Di2 y2,  q = D^-1 y
        double s[3], y[3];
        rt_sym_vec(Di2, y2, s);
        for (int i = 0; i < 3; ++i) y[i] = n.rhs[i] - (E1[i * 3] * y1[0] + E1[i * 3 + 1] * y1[1] + E1[i * 3 + 2] * y1[2]) - c2 * s[i];
        rt_sym_vec(Di, y, q);
        for (int i = 0; i < 6; ++i) {
            Di2[i] = Di1[i];
            Di1[i] = Di[i];
        }
        for (int i = 0; i < 9; ++i) {
            M1[i] = M[i];
            E1[i] = E[i];
        }
        for (int i = 0; i < 3; ++i) {
            y2[i] = y1[i];
            y1[i] = y[i];
        }
        c2 = c1;
        c1 = c;
    }
};
