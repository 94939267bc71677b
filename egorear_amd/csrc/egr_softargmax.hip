// Soft-argmax heat-map decoding: forward, backward and the coordinate L1 loss that seeds it.
// get_max_preds_soft_pytorch (utils/loss.py:145-177) and integrate_tensor_2d (utils/util.py:80-109) as ONE pass over a map:
// one wave owns one (H, W) map, four maps per 256-thread workgroup (argmax_kernel's mapping), reductions by wave butterflies in a
// fixed order - a map's result does not depend on its neighbours in the batch, and no atomics are used anywhere.
//
// Numerics.  With z = beta * h and m = max z = beta * max h (beta > 0), e_i = exp(fma(beta, h_i, -m)) <= 1: nothing overflows
// whatever beta and the peak are, and the rounding of m is common to the whole map (it cancels in e_i / sum e).  The moments are
// taken about the hard arg-max (cm, rm):  x = cm + sum e_i (col_i - cm) / sum e_i,  which keeps the summed terms small where the
// map is peaked (beta 100: the offset is a fraction of a pixel).  The backward recomputes e_i from the same expression and the
// forward's `stat` = (m, sum e), so its p_i are the forward's.
#include "egr_common.h"
#include <math.h>

// every product and sum below is rounded as written (the fused ones are explicit fmaf calls): accumulate = 1 then gives exactly the
// overwrite result plus the prior buffer
#pragma clang fp contract(off)

namespace {

constexpr int SA_REG_MAX = 4096;            // floats of a map that one wave keeps in registers: 16 x 16 bytes per lane
constexpr int SA_CHUNKS = SA_REG_MAX / 256;
constexpr int SA_NONE = 0x7fffffff;

// cross-lane: larger value wins, ties go to the smaller flat index (argmax_kernel's rule); every lane ends with the result
__device__ __forceinline__ void sa_wave_argmax(float& best, int& bidx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(best, o, 64);
        int oi = __shfl_xor(bidx, o, 64);
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
    }
}

// (col, row) of a flat index that advances by a fixed step: one division per lane, none per element
struct sa_walk {
    int col, row, wid, qs, rs;
    __device__ __forceinline__ sa_walk(int idx0, int step, int w) : wid(w) {
        row = idx0 / w;
        col = idx0 - row * w;
        qs = step / w;
        rs = step - qs * w;
    }
    __device__ __forceinline__ void advance() {
        col += rs;
        row += qs;
        if (col >= wid) { col -= wid; ++row; }
    }
};

template <int MODE>
__device__ __forceinline__ float sa_weight(float h, float beta, float zmax) {
    if (MODE == 0) return __expf(fmaf(beta, h, -zmax));
    return fmaxf(beta * h, 0.f);
}

__device__ __forceinline__ void sa_finish(int row, int lane, int hgt, int wid, int normalize, float thr, float best, int bidx, float zmax,
                                          float s, float sx, float sy, float* coords, float* maxvals, int32_t* index, uint8_t* valid,
                                          float* stat) {
    if (lane != 0) return;
    const int rm = bidx / wid, cm = bidx - rm * wid;
    float x = (float)cm + sx / s, y = (float)rm + sy / s;       // mode 1 on a map without positive mass: 0 / 0 = NaN, as the reference
    if (normalize) { x = x / (float)wid; y = y / (float)hgt; }
    coords[(int64_t)row * 2 + 0] = x;
    coords[(int64_t)row * 2 + 1] = y;
    maxvals[row] = best;
    index[row] = bidx;
    valid[row] = best >= thr ? 1 : 0;
    stat[(int64_t)row * 2 + 0] = zmax;
    stat[(int64_t)row * 2 + 1] = s;
}

// ------------------------------------------------------------------ forward, the map in registers
// hw <= 4096, hw % 4 == 0, 16-byte aligned maps: ONE read with 16-byte loads.  POW2: wid is a power of two >= 4, so a 4-element chunk
// never crosses a map row and (col, row) are a mask and a shift of the flat index; otherwise wid >= 4 and the walker wraps once.
template <bool POW2, int MODE, bool PROBS>
__global__ __launch_bounds__(256) void soft_argmax_reg_kernel(const float* hm, int rows, int hgt, int wid, int lw, float beta, int normalize,
                                                              float thr, float* coords, float* maxvals, int32_t* index, uint8_t* valid,
                                                              float* stat, float* probs) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int hw = hgt * wid;
    const float* p = hm + (int64_t)row * hw;
    f32x4 v[SA_CHUNKS];
#pragma unroll
    for (int k = 0; k < SA_CHUNKS; ++k) {
        const int base = k * 256 + lane * 4;
        if (base < hw) v[k] = *reinterpret_cast<const f32x4*>(p + base);      // hw % 4 == 0: a chunk is whole or absent
        else v[k] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};      // weighs exp(-inf) = relu(-inf) = 0
    }
    float best = -INFINITY;
    int bidx = SA_NONE;
    // each lane walks its indices in increasing order, so '>' keeps the first maximum it sees
#pragma unroll
    for (int k = 0; k < SA_CHUNKS; ++k) {
        const int base = k * 256 + lane * 4;
        if (base < hw) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v[k][i] > best || bidx == SA_NONE) { best = v[k][i]; bidx = base + i; }
        }
    }
    sa_wave_argmax(best, bidx);
    const float zmax = beta * best;
    const int rm = bidx / wid, cm = bidx - rm * wid;
    float s = 0.f, sx = 0.f, sy = 0.f;
    sa_walk pos(lane * 4, 256, wid);
#pragma unroll
    for (int k = 0; k < SA_CHUNKS; ++k) {
        if (k * 256 < hw) {                    // wave-uniform: small maps skip the empty passes
            const int base = k * 256 + lane * 4;
            int c = POW2 ? (base & (wid - 1)) : pos.col, r = POW2 ? (base >> lw) : pos.row;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = sa_weight<MODE>(v[k][i], beta, zmax);
                if (PROBS) v[k][i] = e;
                s += e;
                sx = fmaf(e, (float)(c - cm), sx);
                sy = fmaf(e, (float)(r - rm), sy);
                ++c;
                if (!POW2 && c >= wid) { c -= wid; ++r; }
            }
            if (!POW2) pos.advance();
        }
    }
    s = wave_sum(s);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    sa_finish(row, lane, hgt, wid, normalize, thr, best, bidx, zmax, s, sx, sy, coords, maxvals, index, valid, stat);
    if (PROBS) {
        float* q = probs + (int64_t)row * hw;
        const float inv = MODE == 0 ? 1.0f / s : 1.0f;       // mode 1 returns relu(z) as it is (util.py:89, 109)
#pragma unroll
        for (int k = 0; k < SA_CHUNKS; ++k) {
            const int base = k * 256 + lane * 4;
            if (base < hw) *reinterpret_cast<f32x4*>(q + base) = v[k] * inv;
        }
    }
}

// ------------------------------------------------------------------ forward, any other map (hw < 2^24)
// hw % 4 != 0 leaves the maps unaligned: scalar loads, lane l reads l, l + 64, ...; the map is read twice (three times with probs).
template <int MODE>
__global__ __launch_bounds__(256) void soft_argmax_gen_kernel(const float* hm, int rows, int hgt, int wid, float beta, int normalize, float thr,
                                                              float* coords, float* maxvals, int32_t* index, uint8_t* valid, float* stat,
                                                              float* probs) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int hw = hgt * wid;
    const float* p = hm + (int64_t)row * hw;
    float best = -INFINITY;
    int bidx = SA_NONE;
    for (int idx = lane; idx < hw; idx += 64) {
        const float h = p[idx];
        if (h > best || bidx == SA_NONE) { best = h; bidx = idx; }
    }
    sa_wave_argmax(best, bidx);
    const float zmax = beta * best;
    const int rm = bidx / wid, cm = bidx - rm * wid;
    float s = 0.f, sx = 0.f, sy = 0.f;
    sa_walk pos(lane, 64, wid);
    for (int idx = lane; idx < hw; idx += 64) {
        const float e = sa_weight<MODE>(p[idx], beta, zmax);
        s += e;
        sx = fmaf(e, (float)(pos.col - cm), sx);
        sy = fmaf(e, (float)(pos.row - rm), sy);
        pos.advance();
    }
    s = wave_sum(s);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    sa_finish(row, lane, hgt, wid, normalize, thr, best, bidx, zmax, s, sx, sy, coords, maxvals, index, valid, stat);
    if (probs) {
        float* q = probs + (int64_t)row * hw;
        const float inv = MODE == 0 ? 1.0f / s : 1.0f;
        for (int idx = lane; idx < hw; idx += 64) q[idx] = sa_weight<MODE>(p[idx], beta, zmax) * inv;
    }
}

// ------------------------------------------------------------------ backward
// g_hm[i] = beta p_i ((col_i - x) gx + (row_i - y) gy) (+ g_maxvals at the arg-max); every element is written by exactly one lane.
struct sa_bwd_row {
    float zmax, scale, x, y, gx, gy, gm;
    int bidx;
    bool dead;
};

template <int MODE>
__device__ __forceinline__ sa_bwd_row sa_bwd_load(int row, int hgt, int wid, float beta, int normalize, const float* stat, const float* coords,
                                                  const int32_t* index, const float* g_coords, const float* g_maxvals) {
    sa_bwd_row r;
    r.zmax = stat[(int64_t)row * 2 + 0];
    const float s = stat[(int64_t)row * 2 + 1];
    r.x = coords[(int64_t)row * 2 + 0];
    r.y = coords[(int64_t)row * 2 + 1];
    r.gx = g_coords[(int64_t)row * 2 + 0];
    r.gy = g_coords[(int64_t)row * 2 + 1];
    if (normalize) {
        r.x *= (float)wid;
        r.y *= (float)hgt;
        r.gx /= (float)wid;
        r.gy /= (float)hgt;
    }
    r.gm = g_maxvals ? g_maxvals[row] : 0.f;
    r.bidx = index[row];                 // compared with flat indices only, never used as an address
    r.dead = MODE == 1 && !(s > 0.f);    // a map without positive mass: zeros (the reference's autograd gives NaN)
    r.scale = r.dead ? 0.f : beta / s;
    return r;
}

template <int MODE>
__device__ __forceinline__ float sa_bwd_elem(const sa_bwd_row& r, float h, float beta, int c, int rw, int idx) {
    const float t = fmaf((float)c - r.x, r.gx, ((float)rw - r.y) * r.gy);
    float g;
    if (MODE == 0) g = __expf(fmaf(beta, h, -r.zmax)) * r.scale * t;
    else g = (!r.dead && beta * h > 0.f) ? r.scale * t : 0.f;
    return idx == r.bidx ? g + r.gm : g;
}

// hw % 4 == 0 and 16-byte aligned maps of both tensors, wid >= 4: 16-byte loads and stores, any hw
template <bool POW2, int MODE>
__global__ __launch_bounds__(256) void soft_argmax_bwd_vec_kernel(const float* hm, const float* stat, const float* coords, const int32_t* index,
                                                                  const float* g_coords, const float* g_maxvals, int rows, int hgt, int wid,
                                                                  int lw, float beta, int normalize, int accumulate, float* g_hm) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int hw = hgt * wid;
    const float* p = hm + (int64_t)row * hw;
    float* q = g_hm + (int64_t)row * hw;
    const sa_bwd_row r = sa_bwd_load<MODE>(row, hgt, wid, beta, normalize, stat, coords, index, g_coords, g_maxvals);
    sa_walk pos(lane * 4, 256, wid);
#pragma unroll 4
    for (int base = lane * 4; base < hw; base += 256) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(p + base);
        f32x4 g;
        int c = POW2 ? (base & (wid - 1)) : pos.col, rw = POW2 ? (base >> lw) : pos.row;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            g[i] = sa_bwd_elem<MODE>(r, h[i], beta, c, rw, base + i);
            ++c;
            if (!POW2 && c >= wid) { c -= wid; ++rw; }
        }
        if (!POW2) pos.advance();
        if (accumulate) g += *reinterpret_cast<const f32x4*>(q + base);
        *reinterpret_cast<f32x4*>(q + base) = g;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void soft_argmax_bwd_gen_kernel(const float* hm, const float* stat, const float* coords, const int32_t* index,
                                                                  const float* g_coords, const float* g_maxvals, int rows, int hgt, int wid,
                                                                  float beta, int normalize, int accumulate, float* g_hm) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int hw = hgt * wid;
    const float* p = hm + (int64_t)row * hw;
    float* q = g_hm + (int64_t)row * hw;
    const sa_bwd_row r = sa_bwd_load<MODE>(row, hgt, wid, beta, normalize, stat, coords, index, g_coords, g_maxvals);
    sa_walk pos(lane, 64, wid);
    for (int idx = lane; idx < hw; idx += 64) {
        float g = sa_bwd_elem<MODE>(r, p[idx], beta, pos.col, pos.row, idx);
        if (accumulate) g += q[idx];
        q[idx] = g;
        pos.advance();
    }
}

// ------------------------------------------------------------------ coordinate L1 loss and its seed gradient
// loss = w / max(N, 1) * sum over valid maps of |x^ - x*| + |y^ - y*|, (x*, y*) = (index % wid, index / wid); one workgroup, fp64
// sums in a fixed order: thread (maps t, t + 256, ... in order), wave butterfly, the four waves in wave order.
__global__ __launch_bounds__(256) void coord_l1_kernel(const float* coords, const int32_t* index, const uint8_t* valid, int rows, int wid,
                                                       float weight, double* loss, float* g_coords) {
    __shared__ double s_sum[4];
    __shared__ int s_cnt[4];
    const int t = threadIdx.x;
    double acc = 0.0;
    int cnt = 0;
    for (int r = t; r < rows; r += 256) {
        if (!valid[r]) continue;
        const int ti = index[r], ty = ti / wid, tx = ti - ty * wid;
        acc += fabs((double)coords[(int64_t)r * 2] - (double)tx) + fabs((double)coords[(int64_t)r * 2 + 1] - (double)ty);
        ++cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((t & 63) == 0) { s_sum[t >> 6] = acc; s_cnt[t >> 6] = cnt; }
    __syncthreads();
    const double total = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    const int n = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const double per = (double)weight / (double)(n > 0 ? n : 1);
    if (t == 0) loss[0] = per * total;
    if (!g_coords) return;
    const float gs = (float)per;
    for (int r = t; r < rows; r += 256) {
        float gx = 0.f, gy = 0.f;
        if (valid[r]) {
            const int ti = index[r], ty = ti / wid, tx = ti - ty * wid;
            const float dx = coords[(int64_t)r * 2] - (float)tx, dy = coords[(int64_t)r * 2 + 1] - (float)ty;
            gx = dx > 0.f ? gs : (dx < 0.f ? -gs : 0.f);
            gy = dy > 0.f ? gs : (dy < 0.f ? -gs : 0.f);
        }
        g_coords[(int64_t)r * 2] = gx;
        g_coords[(int64_t)r * 2 + 1] = gy;
    }
}

inline bool sa_shape_ok(int32_t rows, int32_t hgt, int32_t wid, float beta, int32_t mode) {
    return rows > 0 && hgt > 0 && wid > 0 && (int64_t)hgt * wid < (1 << 24) && (mode == 0 || mode == 1) && beta > 0.f && beta <= 3.0e38f;
}

inline bool sa_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int sa_log2(int32_t w) {
    int l = 0;
    while ((1 << l) < w) ++l;
    return l;
}

}  // namespace

extern "C" int egr_soft_argmax_f32(const float* hm, int32_t rows, int32_t hgt, int32_t wid, float beta, int32_t mode, int32_t normalize,
                                   float thr, float* coords, float* maxvals, int32_t* index, uint8_t* valid, float* stat, float* probs,
                                   void* stream) {
    if (!hm || !coords || !maxvals || !index || !valid || !stat) return EGR_ENULL;
    if (!sa_shape_ok(rows, hgt, wid, beta, mode)) return EGR_EINVAL;
    const int hw = hgt * wid;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const bool reg = hw <= SA_REG_MAX && hw % 4 == 0 && wid >= 4 && sa_aligned(hm) && (!probs || sa_aligned(probs));
    if (reg) {
        const bool pow2 = (wid & (wid - 1)) == 0;
        const int lw = sa_log2(wid);
#define SA_FWD(P2, M, PR)                                                                                                              \
    hipLaunchKernelGGL((soft_argmax_reg_kernel<P2, M, PR>), grid, block, 0, s, hm, rows, hgt, wid, lw, beta, normalize, thr, coords, \
                       maxvals, index, valid, stat, probs)
        switch ((pow2 ? 4 : 0) | (mode ? 2 : 0) | (probs ? 1 : 0)) {
            case 0: SA_FWD(false, 0, false); break;
            case 1: SA_FWD(false, 0, true); break;
            case 2: SA_FWD(false, 1, false); break;
            case 3: SA_FWD(false, 1, true); break;
            case 4: SA_FWD(true, 0, false); break;
            case 5: SA_FWD(true, 0, true); break;
            case 6: SA_FWD(true, 1, false); break;
            default: SA_FWD(true, 1, true); break;
        }
#undef SA_FWD
    } else if (mode == 0) {
        hipLaunchKernelGGL(soft_argmax_gen_kernel<0>, grid, block, 0, s, hm, rows, hgt, wid, beta, normalize, thr, coords, maxvals, index,
                           valid, stat, probs);
    } else {
        hipLaunchKernelGGL(soft_argmax_gen_kernel<1>, grid, block, 0, s, hm, rows, hgt, wid, beta, normalize, thr, coords, maxvals, index,
                           valid, stat, probs);
    }
    return egr_launch_status();
}

extern "C" int egr_soft_argmax_bwd_f32(const float* hm, const float* stat, const float* coords, const int32_t* index, const float* g_coords,
                                       const float* g_maxvals, int32_t rows, int32_t hgt, int32_t wid, float beta, int32_t mode,
                                       int32_t normalize, int32_t accumulate, float* g_hm, void* stream) {
    if (!hm || !stat || !coords || !index || !g_coords || !g_hm) return EGR_ENULL;
    if (!sa_shape_ok(rows, hgt, wid, beta, mode)) return EGR_EINVAL;
    const int hw = hgt * wid;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (hw % 4 == 0 && wid >= 4 && sa_aligned(hm) && sa_aligned(g_hm)) {
        const bool pow2 = (wid & (wid - 1)) == 0;
        const int lw = sa_log2(wid);
#define SA_BWD(P2, M)                                                                                                                     \
    hipLaunchKernelGGL((soft_argmax_bwd_vec_kernel<P2, M>), grid, block, 0, s, hm, stat, coords, index, g_coords, g_maxvals, rows, hgt, \
                       wid, lw, beta, normalize, accumulate, g_hm)
        switch ((pow2 ? 2 : 0) | (mode ? 1 : 0)) {
            case 0: SA_BWD(false, 0); break;
            case 1: SA_BWD(false, 1); break;
            case 2: SA_BWD(true, 0); break;
            default: SA_BWD(true, 1); break;
        }
#undef SA_BWD
    } else if (mode == 0) {
        hipLaunchKernelGGL(soft_argmax_bwd_gen_kernel<0>, grid, block, 0, s, hm, stat, coords, index, g_coords, g_maxvals, rows, hgt, wid, beta,
                           normalize, accumulate, g_hm);
    } else {
        hipLaunchKernelGGL(soft_argmax_bwd_gen_kernel<1>, grid, block, 0, s, hm, stat, coords, index, g_coords, g_maxvals, rows, hgt, wid, beta,
                           normalize, accumulate, g_hm);
    }
    return egr_launch_status();
}

extern "C" int egr_coord_l1_f32(const float* coords, const int32_t* index, const uint8_t* valid, int32_t rows, int32_t wid, float weight,
                                double* loss, float* g_coords, void* stream) {
    if (!coords || !index || !valid || !loss) return EGR_ENULL;
    if (rows <= 0 || wid <= 0) return EGR_EINVAL;
    hipLaunchKernelGGL(coord_l1_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, coords, index, valid, rows, wid, weight, loss, g_coords);
    return egr_launch_status();
}
