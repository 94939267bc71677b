// Consensus over candidate peaks.
// Every view brings up to K candidate image points per joint (egr_peaks_f32); a hypothesis is one candidate from each of two views,
// h = (pair(a, b) * K + ka) * K + kb with the pairs in lexicographic order.  Its point is the triangulation's two-ray least-squares
// intersection - the same code, rays::add_ray / factor / ldl_solve of egr_rays.h, with the two scores as weights and the same `ok` -
// projected into every view with the unclamped fisheye_pixel; a view supports it with its best
// score * max(0, 1 - e^2 / tau^2),  e the distance (coords units) between the projection and the candidate.  The winner is
// the largest sum of the views' support among hypotheses that at least `min_views` views support, ties to the smaller h.
//
// One wave per (frame, joint), lanes = hypotheses (6 K^2 <= 96: two passes at K = 4).  The first V * K lanes build the candidates'
// rays once - the trigonometry - and park them in LDS, V more lanes the extrinsics; every lane then solves its pair and projects into
// the V views; one fixed-order butterfly (larger score, ties to the smaller h) picks the winner, whose lane writes the outputs.  fp64
// throughout, as in the triangulation: a score's rounding decides a selection.  No atomics, a pair's bits depend on its own operands only.
#include "egr_rays.h"

namespace {

constexpr int CON_MAX_K = 4;
constexpr int CON_NONE = 0x7fffffff;

struct con_cand {
    double d[3];     // unit ray, camera frame
    double w;        // the score; 0: the candidate does not exist
    double x, y;     // coords units
};

__global__ __launch_bounds__(64) void consensus_kernel(const float* cand, const float* cscore, const int32_t* cindex, const float* cams,
                                                       const float* ctm, int V, int J, int K, float sx, float sy, float tau, int min_views,
                                                       float min_det_ratio, int32_t* choice, float* sel_coords, float* sel_conf,
                                                       float* score, int32_t* inliers, int32_t* hyp) {
    __shared__ con_cand s_c[rays::MAX_V * CON_MAX_K];
    __shared__ double s_R[rays::MAX_V][9], s_t[rays::MAX_V][3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int b = pair / J, j = pair - b * J;
    if (lane < V * K) {
        const int v = lane / K, k = lane - v * K;
        const int64_t at = (((int64_t)b * V + v) * J + j) * K + k;
        rays::ray ry;
        // (threshold 0: the score must be positive and finite, the coordinates finite - make_ray's own test)
        rays::make_ray(cand, cscore, cams + v * rays::REC, at, (double)sx, (double)sy, 0.f, ry);
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
        rays::extrinsics(cams + v * rays::REC, ctm, (int64_t)b * V + v, R, t);
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
        rays::normal_eq n;
        rays::add_ray(s_R[va], s_t[va], ca.d, ca.w, n);
        rays::add_ray(s_R[vb], s_t[vb], cb.d, cb.w, n);
        rays::ldl f;
        if (!rays::factor(n, (double)min_det_ratio, f)) continue;
        double p[3];
        rays::ldl_solve(f, n.rhs, p);
        double total = 0.0;
        int inl = 0, pack = 0;
        for (int v = 0; v < V; ++v) {
            const float* cam = cams + v * rays::REC;
            double q[3];
            rays::apply(s_R[v], s_t[v], p, q);
            double px, py;
            if (!egrf::fisheye_pixel<double, float>(cam + rays::W2C, rays::w2c_degree(cam), (double)cam[1], (double)cam[2], q[0], q[1], q[2],
                                                    &px, &py))
                continue;
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
    if (!rays::shape_ok(B, V, J, sx, sy, min_det_ratio) || K < 1 || K > CON_MAX_K || (int64_t)B * J * V * K >= (1 << 30) ||
        !(max_reproj > 0.f && max_reproj <= 3.0e38f) || min_views < 2 || min_views > V)
        return EGR_EINVAL;
    hipLaunchKernelGGL(consensus_kernel, dim3((unsigned)(B * J)), dim3(64), 0, (hipStream_t)stream, cand, cscore, cindex, cams, ctm, V, J, K,
                       sx, sy, max_reproj, min_views, min_det_ratio, choice, sel_coords, sel_conf, score, inliers, hyp);
    return egr_launch_status();
}
