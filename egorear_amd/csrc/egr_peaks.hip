// Multi-peak heat-map decoding: the K best local maxima of every map, each refined to sub-pixel over a small window.
// One wave owns one (H, W) map, one map per 64-thread workgroup: its 16 KB LDS image lets ten of them share a CU (four maps per
// workgroup, egr_softargmax.hip's mapping, measured 4 % slower on the serving shape).  The map is read from HBM once, with 16-byte
// loads where its shape allows, and parked in LDS (NaN stored as -inf, which is how the statement compares it).  A pixel is tested
// against the score floor from the registers it was loaded into; only the few that pass read their neighbours, from LDS - no
// cross-lane traffic.  Every lane keeps the best four of its own peaks in registers, sorted by (value, smaller flat index); K rounds
// of the fixed-order wave arg-max pop the winners.  The refinement of all winners runs at once: sixteen lanes per peak, each up to
// four of the window's at most 49 elements in a fixed order, then a four-step butterfly of three fp64 sums (fp64: exp(beta (h - m))
// may see a positive argument where the window is wider than the suppression radius, and the coordinates are then the float64
// statement's to an fp32 rounding).  No atomics; a map's bits depend on the map alone.
#include "egr_common.h"
#include <math.h>

namespace {

constexpr int PK_MAX_HW = 4096;            // floats of one map: the wave's LDS image
constexpr int PK_CHUNKS = PK_MAX_HW / 256;
constexpr int PK_MAX_K = 4, PK_MAX_NMS = 3, PK_MAX_REFINE = 3;
constexpr int PK_NONE = 0x7fffffff;

// cross-lane: larger value wins, ties go to the smaller flat index (sa_wave_argmax's rule); every lane ends with the result
__device__ __forceinline__ void pk_wave_argmax(float& best, int& bidx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(best, o, 64);
        int oi = __shfl_xor(bidx, o, 64);
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
    }
}

// sum over the sixteen lanes of a peak's group; every lane of the group ends with the result
__device__ __forceinline__ double pk_group_sum(double v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float pk_canon(float h) { return h != h ? -INFINITY : h; }

// pixel idx of value h (finite, above the floor): if it beats its window, it enters the lane's sorted list
__device__ __forceinline__ void pk_test(const float* m, float h, int idx, int hgt, int wid, int rn, float (&bv)[PK_MAX_K], int (&bi)[PK_MAX_K]) {
    const int r = idx / wid, c = idx - r * wid;
    const int r0 = max(r - rn, 0), r1 = min(r + rn, hgt - 1), c0 = max(c - rn, 0), c1 = min(c + rn, wid - 1);
    bool peak = true;
    for (int y = r0; y <= r1 && peak; ++y) {
        const float* line = m + y * wid;
        for (int x = c0; x <= c1; ++x) {
            const float n = line[x];
            const int ni = y * wid + x;
            // h > n for an earlier neighbour, h >= n for a later one: a plateau keeps its first pixel only
            if (ni < idx ? !(h > n) : (ni > idx && !(h >= n))) peak = false;
        }
    }
    if (!peak) return;
    float cv = h;
    int ci = idx;
#pragma unroll
    for (int s = 0; s < PK_MAX_K; ++s) {
        if (cv > bv[s] || (cv == bv[s] && ci < bi[s])) {
            const float tv = bv[s];
            const int ti = bi[s];
            bv[s] = cv;
            bi[s] = ci;
            cv = tv;
            ci = ti;
        }
    }
}

// VEC: hw % 4 == 0 and 16-byte aligned maps
template <bool VEC>
__global__ __launch_bounds__(64) void peaks_kernel(const float* hm, int rows, int hgt, int wid, int K, int rn, int rr, float beta,
                                                    float min_score, float* coords, float* score, int32_t* index, int32_t* count) {
    __shared__ float m[PK_MAX_HW];
    const int lane = threadIdx.x, row = blockIdx.x;
    const int hw = hgt * wid;
    f32x4 v[VEC ? PK_CHUNKS : 1];
    {
        const float* p = hm + (int64_t)row * hw;
        if (VEC) {
#pragma unroll
            for (int k = 0; k < PK_CHUNKS; ++k) {
                const int base = k * 256 + lane * 4;
                if (base < hw) v[k] = *reinterpret_cast<const f32x4*>(p + base);
            }
#pragma unroll
            for (int k = 0; k < PK_CHUNKS; ++k) {
                const int base = k * 256 + lane * 4;
                if (base < hw) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[k][i] = pk_canon(v[k][i]);
                    *reinterpret_cast<f32x4*>(m + base) = v[k];
                }
            }
        } else {
            for (int idx = lane; idx < hw; idx += 64) m[idx] = pk_canon(p[idx]);
        }
    }
    __syncthreads();

    // ---- the lane's own peaks, best first.  A pixel must be finite and above the score floor (NaN is -inf here and fails both).
    float bv[PK_MAX_K];
    int bi[PK_MAX_K];
#pragma unroll
    for (int s = 0; s < PK_MAX_K; ++s) { bv[s] = -INFINITY; bi[s] = PK_NONE; }
    if (VEC) {
        // which of the lane's 64 pixels pass, as a bit mask built from the registers; the loop then visits those only, in index order
        uint64_t pass = 0;
#pragma unroll
        for (int k = 0; k < PK_CHUNKS; ++k) {
            if (k * 256 + lane * 4 < hw) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (v[k][i] > min_score && v[k][i] < INFINITY) pass |= 1ull << (k * 4 + i);
            }
        }
        while (pass) {
            const int bit = __ffsll((unsigned long long)pass) - 1;
            pass &= pass - 1;
            const int idx = (bit >> 2) * 256 + lane * 4 + (bit & 3);
            pk_test(m, m[idx], idx, hgt, wid, rn, bv, bi);
        }
    } else {
        for (int idx = lane; idx < hw; idx += 64) {
            const float h = m[idx];
            if (h > min_score && h < INFINITY) pk_test(m, h, idx, hgt, wid, rn, bv, bi);
        }
    }

    // ---- K rounds of the wave arg-max pop the winners, best first (wave-uniform values)
    float wv[PK_MAX_K];
    int wi[PK_MAX_K];
    int found = 0;
#pragma unroll
    for (int k = 0; k < PK_MAX_K; ++k) {
        wv[k] = 0.f;
        wi[k] = PK_NONE;
        if (k < K && found == k) {                       // (once a round finds nothing, no later one does)
            float best = bv[0];
            int bidx = bi[0];
            pk_wave_argmax(best, bidx);
            if (bidx != PK_NONE) {
                if (bi[0] == bidx) {                     // the owner drops its head
#pragma unroll
                    for (int s = 0; s + 1 < PK_MAX_K; ++s) { bv[s] = bv[s + 1]; bi[s] = bi[s + 1]; }
                    bv[PK_MAX_K - 1] = -INFINITY;
                    bi[PK_MAX_K - 1] = PK_NONE;
                }
                wv[k] = best;
                wi[k] = bidx;
                ++found;
            }
        }
    }

    // ---- the window refinement: lanes 16 g .. 16 g + 15 take peak g, lane `sub` of them the elements sub, sub + 16, ... in that order
    const int g = lane >> 4, sub = lane & 15;
    float pv = wv[0];
    int pi = wi[0];
#pragma unroll
    for (int k = 1; k < PK_MAX_K; ++k)
        if (g == k) { pv = wv[k]; pi = wi[k]; }
    const bool has = pi != PK_NONE;
    const int side = 2 * rr + 1, win = side * side;
    const int rm = has ? pi / wid : 0, cm = has ? pi - rm * wid : 0;
    const double b64 = (double)beta;
    double e = 0.0, ex = 0.0, ey = 0.0;
    if (has) {
        for (int q = sub; q < win; q += 16) {
            const int qy = q / side, wy = qy - rr, wx = q - qy * side - rr;
            const int py = rm + wy, px = cm + wx;
            if (py >= 0 && py < hgt && px >= 0 && px < wid) {
                const float h = m[py * wid + px];
                if (h > -INFINITY && h < INFINITY) {
                    const double t = exp(b64 * ((double)h - (double)pv));
                    e += t;
                    ex += t * (double)wx;
                    ey += t * (double)wy;
                }
            }
        }
    }
    e = pk_group_sum(e);
    ex = pk_group_sum(ex);
    ey = pk_group_sum(ey);
    if (sub == 0 && g < K) {
        const int64_t o = (int64_t)row * K + g;
        // the peak itself contributes exp(0) = 1: e >= 1
        coords[o * 2 + 0] = has ? (float)((double)cm + ex / e) : 0.f;
        coords[o * 2 + 1] = has ? (float)((double)rm + ey / e) : 0.f;
        score[o] = has ? pv : 0.f;
        index[o] = has ? pi : -1;
    }
    if (lane == 0) count[row] = found;
}

}  // namespace

extern "C" int egr_peaks_f32(const float* hm, int32_t rows, int32_t hgt, int32_t wid, int32_t K, int32_t nms_radius, int32_t refine_radius,
                             float beta, float min_score, float* coords, float* score, int32_t* index, int32_t* count, void* stream) {
    if (!hm || !coords || !score || !index || !count) return EGR_ENULL;
    if (rows <= 0 || hgt <= 0 || wid <= 0 || (int64_t)hgt * wid > PK_MAX_HW || K < 1 || K > PK_MAX_K || nms_radius < 1 ||
        nms_radius > PK_MAX_NMS || refine_radius < 0 || refine_radius > PK_MAX_REFINE || !(beta > 0.f && beta <= 3.0e38f) ||
        !(min_score >= -3.4e38f && min_score <= 3.4e38f))
        return EGR_EINVAL;
    const dim3 grid((unsigned)rows), block(64);
    const bool vec = (hgt * wid) % 4 == 0 && ((uintptr_t)hm & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(peaks_kernel<true>, grid, block, 0, (hipStream_t)stream, hm, rows, hgt, wid, K, nms_radius, refine_radius, beta,
                           min_score, coords, score, index, count);
    else
        hipLaunchKernelGGL(peaks_kernel<false>, grid, block, 0, (hipStream_t)stream, hm, rows, hgt, wid, K, nms_radius, refine_radius, beta,
                           min_score, coords, score, index, count);
    return egr_launch_status();
}
