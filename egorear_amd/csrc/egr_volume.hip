// Volumetric fusion of multi-view heat maps into 3-D joints: forward and backward.
// A cube of G^3 voxels around a coarse centre; every voxel centre is projected into every camera (the projection of egr_fisheye.h,
// unclamped; the camera record and the extrinsics of egr_rays.h), the heat maps are sampled there bilinearly with zero padding, the samples of the
// views are fused with the views' weights, and one 3-D soft-argmax over the cube gives the joint:
//   S_i = sum_v w_v s_{v,i} / sum_v w_v,   P = softmax(beta S),   pose = c + sum_i P_i o_i,   spread^2 = sum_i P_i |o_i - (pose - c)|^2.
//
// One workgroup of 512 threads owns one (frame, joint).  The maps of its views are staged in LDS once (64 KB at 4 x 64 x 64) and all
// gathers go there.  A thread walks the voxels tid, tid + 512, ... with an online softmax - running maximum, sum, weighted mean offset
// and weighted second moment about that mean (Welford / Chan, so a one-hot distribution has a spread of 0, not of cancellation noise) -
// and the 512 records are merged in a fixed order: down the lanes of a wave, then wave 0..7.  No score is stored, no atomics in the
// forward: the same bits run to run, alone or in a batch, eager or replayed.  The arithmetic is fp64 on fp32 operands, outputs are
// rounded to fp32 once: every output is the float64 statement's value to within an fp32 ulp.  (A projection is about 300 fp64
// instructions - sqrt, atan2, a 12-term polynomial, four divisions; the measured rate, DESIGN.md 5o, is what issuing them costs.)
//
// The backward (1024 threads, one workgroup per CU: its two LDS images take 128 KB) recomputes the scores from the maps in LDS with
// the same code - the scores and the maximum have the forward's bits, the sums are merged over twice as many threads and agree with
// the forward's to rounding - and scatters
//   gS_i * w_v / sum w * (bilinear weight),   gS_i = beta P_i ((o_i - (pose - c)) . g_pose) + [i == index] g_peak
// into a second LDS image with fp32 LDS atomic adds (the order of those adds is not fixed: the last bits of g_hm may differ between
// runs), then writes every element of g_hm once with plain stores: no global atomics, no zeroed output needed.
#include "egr_rays.h"

namespace {

constexpr int VOL_MAX_V = rays::MAX_V, VOL_MIN_G = 2, VOL_MAX_G = 32;
constexpr int VOL_MAX_ELEMS = 16384;       // V * H * W floats of one LDS image: the product's four 64 x 64 maps
constexpr int VOL_THREADS = 512, VOL_BWD_THREADS = 1024, VOL_MAX_WAVES = VOL_BWD_THREADS / 64;     // forward, backward workgroup

struct vol_view {          // one per view, in LDS: every lane reads the same address (a broadcast)
    double R[9], t[3];     // p_cam = R p + t, cm (rays::extrinsics)
    double poly[rays::MAX_W2C];     // W2C, widened once
    double cx, cy, W_img, H_img;
    double w;              // the view's weight; 0: excluded
    int npoly, pad;
};

struct vol_acc {           // online softmax record: sums are relative to exp(beta * m)
    double m, s, ox, oy, oz, m2;
    int idx;
};

struct vol_tap {           // one view's sample of one voxel: the LDS index of corner (x0, y0) and the corners' weights
    int at;
    double w00, w10, w01, w11;     // 0: the corner is outside the map, or the view gave no sample
};

__device__ __forceinline__ void vol_make_view(const float* conf, const float* cams, const float* ctm, int b, int v, int j, int V, int J,
                                              float thr, vol_view& o) {
    const float* cam = cams + v * rays::REC;
    const float cf = conf[((int64_t)b * V + v) * J + j];
    o.w = (cf >= thr && cf > 0.f && isfinite(cf)) ? (double)cf : 0.0;
    rays::extrinsics(cam, ctm, (int64_t)b * V + v, o.R, o.t);
    o.npoly = rays::w2c_degree(cam);
    for (int i = 0; i < rays::MAX_W2C; ++i) o.poly[i] = (double)cam[rays::W2C + i];
    o.cx = cam[1];
    o.cy = cam[2];
    o.W_img = cam[3];
    o.H_img = cam[4];
    o.pad = 0;
}

// the sample of view v's map (in LDS at maps + v * H * W) at the projection of the device-frame point p; `tap` describes it for the
// backward.  Corners outside the map count 0, so the sample fades to zero across the border; a non-finite coordinate gives 0.
__device__ __forceinline__ double vol_sample(const float* maps, const vol_view& vw, int v, int H, int W, double px, double py, double pz,
                                             vol_tap& tap) {
    const double qx = vw.R[0] * px + vw.R[1] * py + vw.R[2] * pz + vw.t[0];
    const double qy = vw.R[3] * px + vw.R[4] * py + vw.R[5] * pz + vw.t[1];
    const double qz = vw.R[6] * px + vw.R[7] * py + vw.R[8] * pz + vw.t[2];
    double ix, iy;
    if (!egrf::fisheye_pixel<double, double>(vw.poly, vw.npoly, vw.cx, vw.cy, qx, qy, qz, &ix, &iy)) return 0.0;
    const double x = ix * (double)W / vw.W_img, y = iy * (double)H / vw.H_img;
    if (!(x > -1.0 && x < (double)W && y > -1.0 && y < (double)H)) return 0.0;       // (NaN fails every comparison)
    const double xf = floor(x), yf = floor(y), fx = x - xf, fy = y - yf;
    const int x0 = (int)xf, y0 = (int)yf;                                             // -1 .. W-1, -1 .. H-1
    const bool l = x0 >= 0, r = x0 + 1 < W, t = y0 >= 0, b = y0 + 1 < H;
    const int at = v * H * W + y0 * W + x0;
    const double v00 = (l && t) ? (double)maps[at] : 0.0, v10 = (r && t) ? (double)maps[at + 1] : 0.0;
    const double v01 = (l && b) ? (double)maps[at + W] : 0.0, v11 = (r && b) ? (double)maps[at + W + 1] : 0.0;
    tap.at = at;
    tap.w00 = (l && t) ? (1.0 - fx) * (1.0 - fy) : 0.0;
    tap.w10 = (r && t) ? fx * (1.0 - fy) : 0.0;
    tap.w01 = (l && b) ? (1.0 - fx) * fy : 0.0;
    tap.w11 = (r && b) ? fx * fy : 0.0;
    // (as two interpolations, so that a constant map samples to the constant exactly)
    const double top = v00 + fx * (v10 - v00), bot = v01 + fx * (v11 - v01);
    return top + fy * (bot - top);
}

__device__ __forceinline__ void vol_offset(int i, int G, double cube, double& ox, double& oy, double& oz) {
    const int ixv = i % G, iyv = (i / G) % G, izv = i / (G * G);
    ox = (((double)ixv + 0.5) / (double)G - 0.5) * cube;
    oy = (((double)iyv + 0.5) / (double)G - 0.5) * cube;
    oz = (((double)izv + 0.5) / (double)G - 0.5) * cube;
}

// the fused score of voxel offset o around centre c; taps[v] for the backward
__device__ __forceinline__ double vol_score(const float* maps, const vol_view* views, int V, int H, int W, const double* c, double wsum,
                                            double ox, double oy, double oz, vol_tap* taps) {
    double acc = 0.0;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {      // (rolled: the projection's code once, not four times - 256 VGPRs and spills otherwise)
        taps[v].at = 0;
        taps[v].w00 = taps[v].w10 = taps[v].w01 = taps[v].w11 = 0.0;
        if (views[v].w == 0.0) continue;
        acc += views[v].w * vol_sample(maps, views[v], v, H, W, c[0] + ox, c[1] + oy, c[2] + oz, taps[v]);
    }
    return acc / wsum;
}

__device__ __forceinline__ void vol_acc_add(vol_acc& a, double beta, double S, double ox, double oy, double oz, int i) {
    double e;
    if (S > a.m) {             // a new maximum (the first of equals stays): everything so far shrinks by exp(beta (m - S))
        const double sc = exp(beta * (a.m - S));
        a.s *= sc;
        a.m2 *= sc;
        a.m = S;
        a.idx = i;
        e = 1.0;
    } else {
        e = exp(beta * (S - a.m));
    }
    if (e == 0.0) return;
    const double sn = a.s + e, r = e / sn;
    const double dx = ox - a.ox, dy = oy - a.oy, dz = oz - a.oz;
    a.ox += r * dx;
    a.oy += r * dy;
    a.oz += r * dz;
    a.m2 += e * (dx * (ox - a.ox) + dy * (oy - a.oy) + dz * (oz - a.oz));
    a.s = sn;
}

__device__ __forceinline__ void vol_acc_merge(vol_acc& a, const vol_acc& b, double beta) {
    if (b.s == 0.0) return;    // (a thread without a voxel)
    if (a.s == 0.0) {
        a = b;
        return;
    }
    const double m = a.m > b.m ? a.m : b.m;
    const double ea = exp(beta * (a.m - m)), eb = exp(beta * (b.m - m));
    const double sa = a.s * ea, sb = b.s * eb, s = sa + sb;
    const double dx = b.ox - a.ox, dy = b.oy - a.oy, dz = b.oz - a.oz, r = sb / s;
    a.m2 = a.m2 * ea + b.m2 * eb + (dx * dx + dy * dy + dz * dz) * (sa * r);
    a.ox += r * dx;
    a.oy += r * dy;
    a.oz += r * dz;
    if (b.m > a.m || (b.m == a.m && b.idx < a.idx)) a.idx = b.idx;
    a.m = m;
    a.s = s;
}

// the distribution of one pair: every thread walks its voxels, the records are merged in a fixed order, every thread returns the total
__device__ __forceinline__ vol_acc vol_reduce(const float* maps, const vol_view* views, vol_acc* red, int V, int H, int W, int G,
                                              double cube, double beta, const double* c, double wsum) {
    vol_acc a;
    a.m = -INFINITY;
    a.s = a.ox = a.oy = a.oz = a.m2 = 0.0;
    a.idx = 0x7fffffff;
    const int n = G * G * G;
    vol_tap taps[VOL_MAX_V];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        double ox, oy, oz;
        vol_offset(i, G, cube, ox, oy, oz);
        vol_acc_add(a, beta, vol_score(maps, views, V, H, W, c, wsum, ox, oy, oz, taps), ox, oy, oz, i);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {       // lane l takes lane l + off: lane 0 ends with the wave's 64 records, in a fixed order
        vol_acc o;
        o.m = __shfl_down(a.m, off, 64);
        o.s = __shfl_down(a.s, off, 64);
        o.ox = __shfl_down(a.ox, off, 64);
        o.oy = __shfl_down(a.oy, off, 64);
        o.oz = __shfl_down(a.oz, off, 64);
        o.m2 = __shfl_down(a.m2, off, 64);
        o.idx = __shfl_down(a.idx, off, 64);
        vol_acc_merge(a, o, beta);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    vol_acc total = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) vol_acc_merge(total, red[w], beta);
    return total;
}

// what a pair starts with: the views' records, the weight sum, the centre; false: the pair is not valid
__device__ __forceinline__ bool vol_setup(const float* conf, const float* centers, const float* cams, const float* ctm,
                                          const uint8_t* center_ok, int pair, int V, int J, float thr, vol_view* views, double* c,
                                          double& wsum) {
    const int b = pair / J, j = pair - b * J;
    if (threadIdx.x < V) vol_make_view(conf, cams, ctm, b, threadIdx.x, j, V, J, thr, views[threadIdx.x]);
    __syncthreads();
    int used = 0;
    wsum = 0.0;
    for (int v = 0; v < V; ++v)
        if (views[v].w != 0.0) {
            ++used;
            wsum += views[v].w;
        }
    bool fin = true;
    for (int k = 0; k < 3; ++k) {
        const float cf = centers[(int64_t)pair * 3 + k];
        fin = fin && isfinite(cf);
        c[k] = (double)cf;
    }
    return used >= 2 && fin && (!center_ok || center_ok[pair] != 0);
}

// the maps of the views that carry weight, global -> LDS (vec: 16-byte loads)
__device__ __forceinline__ void vol_stage(const float* hm, const vol_view* views, float* maps, int pair, int V, int J, int HW, bool vec) {
    const int b = pair / J, j = pair - b * J;
    for (int v = 0; v < V; ++v) {
        if (views[v].w == 0.0) continue;
        const float* src = hm + (((int64_t)b * V + v) * J + j) * HW;
        float* dst = maps + v * HW;
        if (vec) {
            for (int i = threadIdx.x; i < HW / 4; i += blockDim.x) ((f32x4*)dst)[i] = ((const f32x4*)src)[i];
        } else {
            for (int i = threadIdx.x; i < HW; i += blockDim.x) dst[i] = src[i];
        }
    }
}

// (four waves per SIMD = 128 VGPRs, so that two workgroups share a CU - the LDS admits two: 8 registers spill to scratch, and the
// launch is a fifth shorter than at the 144 VGPRs and one workgroup per CU the compiler picks unasked: 209 against 264 us at grid 16)
__global__ __launch_bounds__(VOL_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void volume_fuse_kernel(
    const float* hm, const float* conf, const float* centers, const float* cams, const float* ctm, const uint8_t* center_ok, int V, int J,
    int H, int W, int G, float cube, float beta, float thr, int vec, float* pose, float* peak, int32_t* index, float* spread, uint8_t* ok) {
    __shared__ __attribute__((aligned(16))) float maps[VOL_MAX_ELEMS];
    __shared__ vol_view views[VOL_MAX_V];
    __shared__ vol_acc red[VOL_MAX_WAVES];
    const int pair = blockIdx.x;
    double c[3], wsum;
    const bool valid = vol_setup(conf, centers, cams, ctm, center_ok, pair, V, J, thr, views, c, wsum);
    if (!valid) {              // (the same decision in every thread of the workgroup)
        if (threadIdx.x == 0) {
            for (int k = 0; k < 3; ++k) pose[(int64_t)pair * 3 + k] = 0.f;
            peak[pair] = 0.f;
            index[pair] = -1;
            spread[pair] = 0.f;
            ok[pair] = 0;
        }
        return;
    }
    vol_stage(hm, views, maps, pair, V, J, H * W, vec != 0);
    __syncthreads();
    const vol_acc a = vol_reduce(maps, views, red, V, H, W, G, (double)cube, (double)beta, c, wsum);
    if (threadIdx.x == 0) {
        pose[(int64_t)pair * 3 + 0] = (float)(c[0] + a.ox);
        pose[(int64_t)pair * 3 + 1] = (float)(c[1] + a.oy);
        pose[(int64_t)pair * 3 + 2] = (float)(c[2] + a.oz);
        peak[pair] = (float)a.m;
        index[pair] = a.idx;
        const double var = a.m2 / a.s;
        spread[pair] = (float)sqrt(var > 0.0 ? var : 0.0);
        ok[pair] = 1;
    }
}

// (1024 threads: the two LDS images leave room for one workgroup per CU, so the workgroup itself brings the four waves per SIMD -
// 128 VGPRs, the taps of a voxel's views in scratch; 805 against 858 us at grid 16 for 512 threads at 154 VGPRs)
__global__ __launch_bounds__(VOL_BWD_THREADS) void volume_fuse_bwd_kernel(const float* hm, const float* conf, const float* centers,
                                                                          const float* cams, const float* ctm, const uint8_t* center_ok,
                                                                          int V, int J, int H, int W, int G, float cube, float beta,
                                                                          float thr, int vec, const float* g_pose, const float* g_peak,
                                                                          float* g_hm) {
    __shared__ __attribute__((aligned(16))) float maps[VOL_MAX_ELEMS];
    __shared__ __attribute__((aligned(16))) float grad[VOL_MAX_ELEMS];
    __shared__ vol_view views[VOL_MAX_V];
    __shared__ vol_acc red[VOL_MAX_WAVES];
    const int pair = blockIdx.x, HW = H * W;
    const int b = pair / J, j = pair - b * J;
    double c[3], wsum;
    const bool valid = vol_setup(conf, centers, cams, ctm, center_ok, pair, V, J, thr, views, c, wsum);
    for (int i = threadIdx.x; i < V * HW; i += VOL_BWD_THREADS) grad[i] = 0.f;
    if (valid) {
        vol_stage(hm, views, maps, pair, V, J, HW, vec != 0);
        __syncthreads();       // (also: the zeros of grad are in place)
        const vol_acc a = vol_reduce(maps, views, red, V, H, W, G, (double)cube, (double)beta, c, wsum);
        double gp[3] = {0.0, 0.0, 0.0};
        if (g_pose)
            for (int k = 0; k < 3; ++k) gp[k] = (double)g_pose[(int64_t)pair * 3 + k];
        const double gk = g_peak ? (double)g_peak[pair] : 0.0, bt = (double)beta;
        const int n = G * G * G;
        vol_tap taps[VOL_MAX_V];
        for (int i = threadIdx.x; i < n; i += VOL_BWD_THREADS) {
            double ox, oy, oz;
            vol_offset(i, G, (double)cube, ox, oy, oz);
            const double S = vol_score(maps, views, V, H, W, c, wsum, ox, oy, oz, taps);
            const double P = exp(bt * (S - a.m)) / a.s;
            const double gS = bt * P * ((ox - a.ox) * gp[0] + (oy - a.oy) * gp[1] + (oz - a.oz) * gp[2]) + (i == a.idx ? gk : 0.0);
            if (gS == 0.0) continue;
#pragma unroll 1
            for (int v = 0; v < V; ++v) {
                const vol_tap& tp = taps[v];               // (all four weights are 0 where the view gave no sample)
                const double k = gS * views[v].w / wsum;
                if (tp.w00 != 0.0) atomicAdd(&grad[tp.at], (float)(k * tp.w00));
                if (tp.w10 != 0.0) atomicAdd(&grad[tp.at + 1], (float)(k * tp.w10));
                if (tp.w01 != 0.0) atomicAdd(&grad[tp.at + W], (float)(k * tp.w01));
                if (tp.w11 != 0.0) atomicAdd(&grad[tp.at + W + 1], (float)(k * tp.w11));
            }
        }
    }
    __syncthreads();
    for (int v = 0; v < V; ++v) {      // every element of the pair's V maps, once
        float* dst = g_hm + (((int64_t)b * V + v) * J + j) * HW;
        const float* src = grad + v * HW;
        if (vec) {
            for (int i = threadIdx.x; i < HW / 4; i += blockDim.x) ((f32x4*)dst)[i] = ((const f32x4*)src)[i];
        } else {
            for (int i = threadIdx.x; i < HW; i += blockDim.x) dst[i] = src[i];
        }
    }
}

inline bool vol_shape_ok(int32_t B, int32_t V, int32_t J, int32_t H, int32_t W, int32_t G, float cube, float beta, float thr) {
    return B > 0 && J > 0 && H > 0 && W > 0 && V >= 2 && V <= VOL_MAX_V && G >= VOL_MIN_G && G <= VOL_MAX_G && H <= VOL_MAX_ELEMS &&
           W <= VOL_MAX_ELEMS && (int64_t)V * H * W <= VOL_MAX_ELEMS && (int64_t)B * J < (1 << 30) && cube > 0.f && cube <= 3.0e38f &&
           beta > 0.f && beta <= 3.0e38f && thr == thr;
}

}  // namespace

extern "C" int egr_volume_fuse_f32(const float* hm, const float* conf, const float* centers, const float* cams, const float* ctm,
                                   const uint8_t* center_ok, int32_t B, int32_t V, int32_t J, int32_t H, int32_t W, int32_t G, float cube,
                                   float beta, float threshold, float* pose, float* peak, int32_t* index, float* spread, uint8_t* ok,
                                   void* stream) {
    if (!hm || !conf || !centers || !cams || !pose || !peak || !index || !spread || !ok) return EGR_ENULL;
    if (!vol_shape_ok(B, V, J, H, W, G, cube, beta, threshold)) return EGR_EINVAL;
    const int vec = (H * W) % 4 == 0 && ((uintptr_t)hm & 15) == 0;
    hipLaunchKernelGGL(volume_fuse_kernel, dim3((unsigned)(B * J)), dim3(VOL_THREADS), 0, (hipStream_t)stream, hm, conf, centers, cams, ctm,
                       center_ok, V, J, H, W, G, cube, beta, threshold, vec, pose, peak, index, spread, ok);
    return egr_launch_status();
}

extern "C" int egr_volume_fuse_bwd_f32(const float* hm, const float* conf, const float* centers, const float* cams, const float* ctm,
                                       const uint8_t* center_ok, int32_t B, int32_t V, int32_t J, int32_t H, int32_t W, int32_t G,
                                       float cube, float beta, float threshold, const float* g_pose, const float* g_peak, float* g_hm,
                                       void* stream) {
    if (!hm || !conf || !centers || !cams || !g_hm) return EGR_ENULL;
    if (!vol_shape_ok(B, V, J, H, W, G, cube, beta, threshold)) return EGR_EINVAL;
    const int vec = (H * W) % 4 == 0 && ((uintptr_t)hm & 15) == 0 && ((uintptr_t)g_hm & 15) == 0;
    hipLaunchKernelGGL(volume_fuse_bwd_kernel, dim3((unsigned)(B * J)), dim3(VOL_BWD_THREADS), 0, (hipStream_t)stream, hm, conf, centers, cams,
                       ctm, center_ok, V, J, H, W, G, cube, beta, threshold, vec, g_pose, g_peak, g_hm);
    return egr_launch_status();
}
