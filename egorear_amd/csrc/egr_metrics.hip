// Pose evaluation metrics on the device (a25 is the path's parity metric).
// Replaces evaluate_pose of pl_wrappers/egoposeformer/pose_3d_mvf_ex.py:317-333, i.e.
//   compute_mpjpe_batch / compute_pck_3d_batch / compute_auc_3d_batch   (utils/loss.py:9-48)
//   batch_compute_similarity_transform_numpy -> compute_similarity_transform (models/utils/pose_metric.py:104-167),
// which the reference runs on the host with one numpy SVD per sample after a device-to-host copy.
// One thread per sample: 16 joints, a 3x3 cross-covariance, its SVD by cyclic Jacobi on K^T K in fp64 (tiny work;
// fp64 keeps the rotation accurate to fp32 round-off whatever the conditioning).
#include "egr_common.h"

namespace {

constexpr int MAXJ = 32;

__device__ void jacobi_eig3(double a[3][3], double v[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(a[p][q]) < 1e-300) continue;
                double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {  // A <- A J
                    double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {  // A <- J^T A
                    double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {  // V <- V J
                    double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

__device__ double det3(const double m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

__global__ __launch_bounds__(64) void pose_metrics_kernel(const float* pred, const float* gt, int B, int J, float pck_thr_mm,
                                                          int n_auc, float* out, float* aligned) {
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float* P = pred + (int64_t)b * J * 3;
    const float* G = gt + (int64_t)b * J * 3;
    // ---- MPJPE, PCK, AUC on the raw prediction (cm -> mm by x10 on each operand, as the reference does)
    float sum_err = 0.f;
    float dmm[MAXJ];
    for (int j = 0; j < J; ++j) {
        // no FMA contraction here: each cm->mm product is rounded to fp32 before the subtraction, as in the reference,
        // so a perfect prediction has distance exactly 0 and passes the threshold-0 bin of the AUC
#pragma clang fp contract(off)
        float dx = P[3 * j] - G[3 * j], dy = P[3 * j + 1] - G[3 * j + 1], dz = P[3 * j + 2] - G[3 * j + 2];
        sum_err += sqrtf(dx * dx + dy * dy + dz * dz);
        float gx = G[3 * j] * 10.f, gy = G[3 * j + 1] * 10.f, gz = G[3 * j + 2] * 10.f;
        float px = P[3 * j] * 10.f, py = P[3 * j + 1] * 10.f, pz = P[3 * j + 2] * 10.f;
        float ex = gx - px, ey = gy - py, ez = gz - pz;
        dmm[j] = sqrtf(ex * ex + ey * ey + ez * ez);
    }
    float mpjpe_mm = sum_err / (float)J * 10.f;
    int correct = 0;
    for (int j = 0; j < J; ++j) correct += dmm[j] <= pck_thr_mm;
    float pck = (float)correct / (float)J * 100.f;
    float auc = 0.f;
    for (int t = 0; t < n_auc; ++t) {  // thresholds linspace(0, pck_thr, n_auc)
        float thr = (n_auc > 1) ? pck_thr_mm * (float)t / (float)(n_auc - 1) : pck_thr_mm;
        int c = 0;
        for (int j = 0; j < J; ++j) c += dmm[j] <= thr;
        auc += (float)c / (float)J;
    }
    auc = auc / (float)n_auc * 100.f;
    // ---- similarity (Procrustes) alignment of pred onto gt: compute_similarity_transform
    double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
    for (int j = 0; j < J; ++j)
        for (int c = 0; c < 3; ++c) {
            mu1[c] += P[3 * j + c];
            mu2[c] += G[3 * j + c];
        }
    for (int c = 0; c < 3; ++c) { mu1[c] /= J; mu2[c] /= J; }
    double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
    for (int j = 0; j < J; ++j) {
        double x1[3], x2[3];
        for (int c = 0; c < 3; ++c) { x1[c] = P[3 * j + c] - mu1[c]; x2[c] = G[3 * j + c] - mu2[c]; var1 += x1[c] * x1[c]; }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K[r][c] += x1[r] * x2[c];  // K = X1 X2^T
    }
    // SVD of K via eigen-decomposition of K^T K = V S^2 V^T;  U = K V S^-1
    double A[3][3], V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r][c] = K[0][r] * K[0][c] + K[1][r] * K[1][c] + K[2][r] * K[2][c];
    jacobi_eig3(A, V);
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j2 = i + 1; j2 < 3; ++j2)
            if (A[ord[j2]][ord[j2]] > A[ord[i]][ord[i]]) { int t = ord[i]; ord[i] = ord[j2]; ord[j2] = t; }
    double Vs[3][3], U[3][3], sv[3];
    for (int i = 0; i < 3; ++i) {
        sv[i] = sqrt(fmax(A[ord[i]][ord[i]], 0.0));
        for (int r = 0; r < 3; ++r) Vs[r][i] = V[r][ord[i]];
    }
    for (int i = 0; i < 3; ++i) {
        double u[3] = {K[0][0] * Vs[0][i] + K[0][1] * Vs[1][i] + K[0][2] * Vs[2][i],
                       K[1][0] * Vs[0][i] + K[1][1] * Vs[1][i] + K[1][2] * Vs[2][i],
                       K[2][0] * Vs[0][i] + K[2][1] * Vs[1][i] + K[2][2] * Vs[2][i]};
        double nrm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        if (nrm > 1e-12 * (sv[0] + 1e-300) && i < 2) {
            for (int r = 0; r < 3; ++r) U[r][i] = u[r] / nrm;
        } else if (i == 2) {
            // third left singular vector: use K v / s when well defined, else complete the basis
            if (nrm > 1e-9 * (sv[0] + 1e-300)) for (int r = 0; r < 3; ++r) U[r][2] = u[r] / nrm;
            else {
                U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
                U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
                U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
            }
        } else {
            for (int r = 0; r < 3; ++r) U[r][i] = (r == i) ? 1.0 : 0.0;
        }
    }
    // Z fixes det(R) = +1: Z = diag(1, 1, sign(det(U V^T)));  R = V Z U^T
    double UVt[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) UVt[r][c] = U[r][0] * Vs[c][0] + U[r][1] * Vs[c][1] + U[r][2] * Vs[c][2];
    double dt = det3(UVt);
    double z = dt > 0 ? 1.0 : (dt < 0 ? -1.0 : 0.0);
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = Vs[r][0] * U[c][0] + Vs[r][1] * U[c][1] + z * Vs[r][2] * U[c][2];
    double trRK = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) trRK += R[r][c] * K[c][r];
    double scale = trRK / var1;
    double tvec[3];
    for (int r = 0; r < 3; ++r) tvec[r] = mu2[r] - scale * (R[r][0] * mu1[0] + R[r][1] * mu1[1] + R[r][2] * mu1[2]);
    float pa_sum = 0.f;
    for (int j = 0; j < J; ++j) {
        float h[3];
        for (int r = 0; r < 3; ++r)
            h[r] = (float)(scale * (R[r][0] * P[3 * j] + R[r][1] * P[3 * j + 1] + R[r][2] * P[3 * j + 2]) + tvec[r]);
        if (aligned) { aligned[((int64_t)b * J + j) * 3 + 0] = h[0]; aligned[((int64_t)b * J + j) * 3 + 1] = h[1]; aligned[((int64_t)b * J + j) * 3 + 2] = h[2]; }
        float dx = h[0] - G[3 * j], dy = h[1] - G[3 * j + 1], dz = h[2] - G[3 * j + 2];
        pa_sum += sqrtf(dx * dx + dy * dy + dz * dz);
    }
    out[4 * b + 0] = mpjpe_mm;
    out[4 * b + 1] = pa_sum / (float)J * 10.f;
    out[4 * b + 2] = pck;
    out[4 * b + 3] = auc;
}

}  // namespace

extern "C" int egr_pose_metrics_f32(const float* pred, const float* gt, int32_t b, int32_t joints, float pck_thr_mm,
                                    int32_t n_auc, float* out, float* aligned, void* stream) {
    if (!pred || !gt || !out) return EGR_ENULL;
    if (b <= 0 || joints <= 0 || joints > MAXJ || n_auc <= 0) return EGR_EINVAL;
    hipLaunchKernelGGL(pose_metrics_kernel, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pred, gt, b, joints,
                       pck_thr_mm, n_auc, out, aligned);
    return egr_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------
// Ground-truth heat-map synthesis: replaces generate_target of generate_heatmap.py:10-48
// (offline numpy loop writing one .npy per frame and camera).  One workgroup per (sample, joint) map: zero fill and a
// (2*tmp+1)^2 Gaussian window centred on int(x / stride + 0.5), clipped to the map; the window table is computed on the
// host with numpy float32 exactly as the reference does, so values are bit-identical.
namespace {
__global__ __launch_bounds__(256) void gt_heatmap_kernel(const double* joints, int maps, double stride, int hs, int tmp,
                                                         const float* gauss, float* out) {
    const int map = blockIdx.x;
    if (map >= maps) return;
    float* o = out + (int64_t)map * hs * hs;
    const double jx = joints[2 * map], jy = joints[2 * map + 1];
    const int mu_x = (int)(jx / stride + 0.5), mu_y = (int)(jy / stride + 0.5);   // C cast == Python int(): toward zero
    const int ulx = mu_x - tmp, uly = mu_y - tmp, brx = mu_x + tmp + 1, bry = mu_y + tmp + 1;
    const bool visible = !(ulx >= hs || uly >= hs || brx < 0 || bry < 0);
    const int size = 2 * tmp + 1;
    for (int i = threadIdx.x; i < hs * hs; i += 256) {
        int y = i / hs, x = i - y * hs;
        float v = 0.f;
        if (visible && x >= ulx && x < brx && y >= uly && y < bry) v = gauss[(y - uly) * size + (x - ulx)];
        o[i] = v;
    }
}
}  // namespace

extern "C" int egr_gt_heatmap_f32(const double* joints, int32_t maps, double image_size, int32_t heatmap_size, int32_t tmp_size,
                                  const float* gauss, float* out, void* stream) {
    if (!joints || !gauss || !out) return EGR_ENULL;
    if (maps <= 0 || heatmap_size <= 0 || tmp_size < 0 || image_size <= 0) return EGR_EINVAL;
    hipLaunchKernelGGL(gt_heatmap_kernel, dim3((unsigned)maps), dim3(256), 0, (hipStream_t)stream, joints, maps,
                       image_size / (double)heatmap_size, heatmap_size, tmp_size, gauss, out);
    return egr_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------
// Heat-map validation metrics: replaces `evaluate` of pl_wrappers/egoposeformer/heatmap.py:220-254 and
// heatmap_mvf_ex.py:263-316 (get_max_preds: utils/loss.py:122-142) and `evaluate_heatmap` of pose_3d_mvf_ex.py:335-361, which
// the reference runs as a Python loop with one device-to-host copy per sample.
// Phase 1, one workgroup per (b, v, j) map: the ground truth is read once for all `sets` predictions; per set the three sums
// {|p - g|, |p - g| where g > 0, (p - g)^2} are taken in fp64 (the launch is bound by the loads) and the first maximum is tracked
// with the tie rule of argmax_kernel.  Reduction order is fixed: lane, wave butterfly, LDS over the four waves in wave order.
// Phase 2, one workgroup per (set, view group): per sample the per-map partials are added in (view, joint) order, then the
// samples' squared-error sums and the integer point distances go through the same fixed tree.  No atomics anywhere: two runs
// give the same bits.
namespace {

constexpr int HM_MAXS = EGR_HM_MAX_SETS;
constexpr int HM_MAXG = EGR_HM_MAX_GROUPS;

struct hm_args {
    const float* pred[HM_MAXS];
    int32_t v0[HM_MAXG], v1[HM_MAXG];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void hm_take(float v, int i, float& best, int& bidx) {
    if (v > best || bidx == 0x7fffffff) { best = v; bidx = i; }
}

__device__ __forceinline__ void hm_merge(float ov, int oi, float& best, int& bidx) {
    if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
}

__global__ __launch_bounds__(256) void heatmap_partials_kernel(hm_args a, const float* gt, int sets, int maps, int hw, float thr,
                                                               double* partials, int32_t* argmax, float* maxval, uint8_t* valid) {
    const int map = blockIdx.x;
    if (map >= maps) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = (int64_t)map * hw;
    double acc[HM_MAXS][3];
    float best[HM_MAXS + 1];
    int bidx[HM_MAXS + 1];
#pragma unroll
    for (int s = 0; s <= HM_MAXS; ++s) { best[s] = -INFINITY; bidx[s] = 0x7fffffff; }
#pragma unroll
    for (int s = 0; s < HM_MAXS; ++s) acc[s][0] = acc[s][1] = acc[s][2] = 0.0;
    // each thread walks its indices in increasing order, so '>' keeps the first maximum it sees
#pragma unroll 2
    for (int base = tid * 4; base < hw; base += 1024) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(gt + off + base);
#pragma unroll
        for (int i = 0; i < 4; ++i) hm_take(g[i], base + i, best[HM_MAXS], bidx[HM_MAXS]);
#pragma unroll
        for (int s = 0; s < HM_MAXS; ++s) {
            if (s < sets) {
                const f32x4 p = *reinterpret_cast<const f32x4*>(a.pred[s] + off + base);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double d = fabs((double)p[i] - (double)g[i]);
                    acc[s][0] += d;
                    acc[s][1] += g[i] > 0.f ? d : 0.0;
                    acc[s][2] += d * d;
                    hm_take(p[i], base + i, best[s], bidx[s]);
                }
            }
        }
    }
    __shared__ double s_acc[4][HM_MAXS * 3];
    __shared__ float s_bv[4][HM_MAXS + 1];
    __shared__ int s_bi[4][HM_MAXS + 1];
#pragma unroll
    for (int s = 0; s < HM_MAXS; ++s) {
        if (s < sets) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double r = wave_sum_f64(acc[s][k]);
                if (lane == 0) s_acc[wave][s * 3 + k] = r;
            }
        }
    }
#pragma unroll
    for (int s = 0; s <= HM_MAXS; ++s) {
        if (s < sets || s == HM_MAXS) {
            float bv = best[s];
            int bi = bidx[s];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                hm_merge(ov, oi, bv, bi);
            }
            if (lane == 0) { s_bv[wave][s] = bv; s_bi[wave][s] = bi; }
        }
    }
    __syncthreads();
    if (tid < sets * 3)
        partials[((int64_t)(tid / 3) * maps + map) * 3 + tid % 3] = ((s_acc[0][tid] + s_acc[1][tid]) + s_acc[2][tid]) + s_acc[3][tid];
    if (tid >= 64 && tid - 64 <= HM_MAXS) {        // (a second wave: the two tails run side by side)
        const int s = tid - 64;
        if (s < sets || s == HM_MAXS) {
            float bv = s_bv[0][s];
            int bi = s_bi[0][s];
            for (int w = 1; w < 4; ++w) hm_merge(s_bv[w][s], s_bi[w][s], bv, bi);
            const int slot = s == HM_MAXS ? sets : s;          // the ground truth's row follows the sets'
            argmax[(int64_t)slot * maps + map] = bi;
            maxval[(int64_t)slot * maps + map] = bv;
            if (s == HM_MAXS) valid[map] = bv >= thr ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void heatmap_finish_kernel(hm_args a, int sets, int groups, int B, int V, int J, int hw, int wid,
                                                             const double* partials, const int32_t* argmax, const uint8_t* valid,
                                                             float* l1, float* pos_l1, float* mse, float* mse_pts) {
    const int s = blockIdx.x / groups, g = blockIdx.x - s * groups;
    if (s >= sets) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v0 = a.v0[g], v1 = a.v1[g];
    const int64_t maps = (int64_t)B * V * J;
    double sse = 0.0;
    long long pts = 0;
    for (int b = tid; b < B; b += 256) {
        double sl1 = 0.0, spos = 0.0, ssq = 0.0;
        for (int v = v0; v < v1; ++v)
            for (int j = 0; j < J; ++j) {
                const int64_t m = ((int64_t)b * V + v) * J + j;
                const double* p = partials + ((int64_t)s * maps + m) * 3;
                sl1 += p[0];
                spos += p[1];
                ssq += p[2];
                if (valid[m]) {        // pts(pred) * valid - pts(gt) * valid: integer pixel coordinates
                    const int pi = argmax[(int64_t)s * maps + m], gi = argmax[(int64_t)sets * maps + m];
                    const int dx = pi % wid - gi % wid, dy = pi / wid - gi / wid;
                    pts += (long long)(dx * dx + dy * dy);
                }
            }
        l1[((int64_t)s * groups + g) * B + b] = (float)sl1;
        pos_l1[((int64_t)s * groups + g) * B + b] = (float)spos;
        sse += ssq;
    }
    __shared__ double s_sse[4];
    __shared__ long long s_pts[4];
    sse = wave_sum_f64(sse);
    pts = wave_sum_i64(pts);
    if (lane == 0) { s_sse[wave] = sse; s_pts[wave] = pts; }
    __syncthreads();
    if (tid == 0) {
        const double n = (double)B * (double)(v1 - v0) * (double)J;
        mse[s * groups + g] = (float)((((s_sse[0] + s_sse[1]) + s_sse[2]) + s_sse[3]) / (n * (double)hw));
        mse_pts[s * groups + g] = (float)((double)(s_pts[0] + s_pts[1] + s_pts[2] + s_pts[3]) / (n * 2.0));
    }
}

}  // namespace

extern "C" int egr_heatmap_metrics_f32(const float* const* preds, int32_t sets, const float* gt, int32_t b, int32_t v, int32_t joints,
                                       int32_t hgt, int32_t wid, const int32_t* view_groups, int32_t n_groups, float threshold,
                                       double* partials, int32_t* argmax, float* maxval, uint8_t* valid, float* l1, float* pos_l1,
                                       float* mse, float* mse_pts2d, void* stream) {
    if (!preds || !gt || !view_groups || !partials || !argmax || !maxval || !valid || !l1 || !pos_l1 || !mse || !mse_pts2d) return EGR_ENULL;
    if (sets < 1 || sets > HM_MAXS || n_groups < 1 || n_groups > HM_MAXG || b <= 0 || v <= 0 || joints <= 0 || joints > MAXJ ||
        hgt <= 0 || wid <= 0)
        return EGR_EINVAL;
    const int64_t hw = (int64_t)hgt * wid, maps = (int64_t)b * v * joints;
    if (hw % 4 != 0 || hw >= (1 << 24) || maps >= (1ll << 31) || ((uintptr_t)gt & 15)) return EGR_EINVAL;
    hm_args a = {};
    for (int s = 0; s < sets; ++s) {
        if (!preds[s]) return EGR_ENULL;
        if ((uintptr_t)preds[s] & 15) return EGR_EINVAL;
        a.pred[s] = preds[s];
    }
    for (int g = 0; g < n_groups; ++g) {
        a.v0[g] = view_groups[2 * g];
        a.v1[g] = view_groups[2 * g + 1];
        if (a.v0[g] < 0 || a.v1[g] > v || a.v0[g] >= a.v1[g]) return EGR_EINVAL;      // (an empty view group is refused)
    }
    hipLaunchKernelGGL(heatmap_partials_kernel, dim3((unsigned)maps), dim3(256), 0, (hipStream_t)stream, a, gt, sets, (int)maps, (int)hw,
                       threshold, partials, argmax, maxval, valid);
    hipLaunchKernelGGL(heatmap_finish_kernel, dim3((unsigned)(sets * n_groups)), dim3(256), 0, (hipStream_t)stream, a, sets, n_groups, b, v,
                       joints, (int)hw, wid, partials, argmax, valid, l1, pos_l1, mse, mse_pts2d);
    return egr_launch_status();
}
