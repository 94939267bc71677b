// The ONE statement of what the conv kernels (egr_conv.hip, egr_conv_tapx.hip, egr_conv_chain.hip) must agree on bit for bit:
// output pixel m -> (image, pixel, row), the x2 bilinear residual (EGR_RES_UP2_BEFORE_ACT), the per-element epilogue value, the
// abs-max fold, the train-mode BatchNorm partials and the point-wise kernels' epilogue row record.
#pragma once
#include "egr_conv_shared.h"
#include "egr_up2.h"

namespace egrc {

constexpr int OOB = (int)0x80000000;   // buffer byte offset beyond every descriptor's range: loads return 0, stores are dropped

// ---- output pixel m -> image n, pixel pix of its HoWo: shifts when ho * wo is a power of two (every layer of the path), multiply-high otherwise
__device__ __forceinline__ void pixel_of(const ConvArgs& a, int m, int HoWo, int& n, int& pix) {
    if (a.howo_shift >= 0) { n = m >> a.howo_shift; pix = m & (HoWo - 1); }
    else { n = fdiv(m, a.dHoWo); pix = m - n * HoWo; }
}
// row of pixel pix in rows of Wenum pixels, and (row_of) its column
__device__ __forceinline__ int row_index(const ConvArgs& a, int pix) { return (a.wo_shift >= 0) ? (pix >> a.wo_shift) : fdiv(pix, a.dWo); }
__device__ __forceinline__ void row_of(const ConvArgs& a, int pix, int Wenum, int& ho, int& wo) {
    if (a.wo_shift >= 0) { ho = pix >> a.wo_shift; wo = pix & (Wenum - 1); }
    else { ho = fdiv(pix, a.dWo); wo = pix - ho * Wenum; }
}
// element offset of image n (32-bit: the host bounds every operand below 2^31 elements); plain: the map is a plain batch
__device__ __forceinline__ int image_offset(const egr_nmap map, int plain, const FastDiv div, int n) {
    return plain ? n * (int)map.stride_inner : (int)fmap(map, div, n);
}

// ---- EGR_RES_UP2_BEFORE_ACT: the residual is the bilinear x2 up-sampling (align_corners = True, egr_up2.h's arithmetic: nothing left
// to the compiler's contraction) of a HALF-resolution tensor.  Output pixel (ho, wo) of a d.ho x d.wo image:
struct Up2Res {
    int off;               // element offset of the upper-left corner relative to the image
    bool last_x, last_y;   // the right / lower neighbour is the same pixel (last column / row)
    float lx1, ly1;        // weights of the right / lower neighbours (the others: 1 - l)
};
// egr_up2::axis with the weight from the ROUNDED product: l1 = clamp(round(s o) - i0).  Not ATen's arithmetic, and not what any other
// site computes: it is what the compiler made of the persistent tiled kernels' decode of their NEXT tile (conv_igemm_x6p_kernel: packed
// multiply, then a subtraction) while it contracted the same text for their first tile.  Kept under this name so that no bit moves.
__device__ __forceinline__ egr_up2::Axis axis_rounded_product(float s, int o, int in) {
#pragma clang fp contract(off)
    egr_up2::Axis a = egr_up2::axis(s, o, in);
    a.l1 = fminf(fmaxf(s * (float)o - (float)a.i0, 0.f), 1.f);
    a.l0 = 1.f - a.l1;
    return a;
}
__device__ __forceinline__ Up2Res up2_res(const egr_conv_desc& d, int ho, int wo, bool rounded_product = false) {
    const int hl = d.ho >> 1, wl = d.wo >> 1;
    const float sy = egr_up2::scale(hl, d.ho), sx = egr_up2::scale(wl, d.wo);
    const egr_up2::Axis ay = rounded_product ? axis_rounded_product(sy, ho, hl) : egr_up2::axis(sy, ho, hl);
    const egr_up2::Axis ax = rounded_product ? axis_rounded_product(sx, wo, wl) : egr_up2::axis(sx, wo, wl);
    return Up2Res{(ay.i0 * wl + ax.i0) * d.ldr, ax.i0 + 1 > wl - 1, ay.i0 + 1 > hl - 1, ax.l1, ay.l1};
}
// t + the residual's value from its four corners (v00 v01 / v10 v11), every contraction written out: the form the parent's ISA shows
// at all four sites.  (The tiled kernels' site still leaves the same expression to the compiler: conv_igemm_body.)
__device__ __forceinline__ float up2_res_add(float t, float v00, float v01, float v10, float v11, float lx1, float ly1) {
#pragma clang fp contract(off)
    const float lx0 = 1.f - lx1, ly0 = 1.f - ly1;
    const float top = __builtin_fmaf(lx0, v00, lx1 * v01);
    const float bot = __builtin_fmaf(lx0, v10, lx1 * v11);
    return t + __builtin_fmaf(ly0, top, ly1 * bot);
}

// ---- the epilogue value of one element: scale / shift [row scale] -> residual before -> activation -> residual after.
// act / res_mode: run-time values or literals (inlined, a literal leaves straight-line code: rows_fast of conv_igemm_body).
// rs = 1 without a row scale, r unused without a residual.  Masks (ReLU mask, row mask) select between this value and 0 at the site.
__device__ __forceinline__ float epi_value(float acc, float sc, float sh, float rs, float r, int act, int res_mode) {
    // (this contraction stays the compiler's: the parent's rows do not agree on it - with a row scale the tiled kernels' generic rows
    // round both products and add, splitk_reduce_kernel and linear_small_kernel fuse - so one written-out form would move bits)
    float t = acc * sc + sh * rs;
    if (res_mode == EGR_RES_BEFORE_ACT) t += r;
    t = egr_act(t, act);
    if (res_mode == EGR_RES_AFTER_ACT) t += r;
    return t;
}

// max |v| of a quad folded into amx
__device__ __forceinline__ void amax4(float& amx, const f32x4& v) {
    amx = fmaxf(fmaxf(amx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
}

// ---- train-mode BatchNorm partials (ConvArgs::bn_part): one element into a channel's running sums (double) and extremes (float) ...
__device__ __forceinline__ void bn_accumulate(float v, double& ds, double& dq, float& lo, float& hi) {
    ds += (double)v;
    dq += (double)v * (double)v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
}
// ... and channel c of M tile tm of group grp into its slab: [groups][tilesM][2][cout] doubles, the extremes as floats behind ALL the sums
__device__ __forceinline__ void bn_store(const ConvArgs& a, int grp, int tm, int c, double ds, double dq, float lo, float hi) {
    const int cout = a.d.cout;
    const int64_t slab = ((int64_t)grp * a.tilesM + tm) * 2 * cout + c;
    float* const mm = reinterpret_cast<float*>(a.bn_part + (int64_t)a.d.groups * a.tilesM * 2 * cout);
    a.bn_part[slab] = ds;
    a.bn_part[slab + cout] = dq;
    mm[slab] = lo;
    mm[slab + cout] = hi;
}

// ---- epilogue rows of the point-wise kernels (conv_pw_x6_body, conv_pw_chain_kernel; conv_pw2_kernel's value): lane p of a wave owns pixel
// m = 32 t + p of the wave's tile; the tile is stored row-major, so the lane that stores a row takes its record from the pixel's owner.
// RESK: 0 no residual, 1 residual of the output's shape, 2 EGR_RES_UP2_BEFORE_ACT.  Byte offsets (buffer addressing), c0 = the
// launch's first output channel; past the last pixel: out of range, loads return zeros and stores are dropped.
struct PwRow {
    int yo, ro, ox, oy;    // output / residual (upper-left corner) byte offsets; RESK 2: byte steps to the right / lower corner (0: same pixel)
    float lx1, ly1;
};
template <int RESK>
__device__ __forceinline__ PwRow pw_row_own(const ConvArgs& a, int m, bool live, int HoWo, int c0) {
    const egr_conv_desc& d = a.d;
    int n, pix;
    pixel_of(a, m, HoWo, n, pix);
    PwRow r = {OOB, OOB, 0, 0, 0.f, 0.f};
    if (live) r.yo = (image_offset(d.ymap, a.y_plain, a.dYin, n) + pix * d.ldy + c0) * 4;
    if (RESK == 1 && live) r.ro = (image_offset(d.rmap, a.r_plain, a.dRin, n) + pix * d.ldr + c0) * 4;
    if constexpr (RESK == 2) {
        int ho, wo;
        row_of(a, pix, d.wo, ho, wo);
        const Up2Res u = up2_res(d, ho, wo);
        r.ly1 = u.ly1; r.lx1 = u.lx1;
        if (live) r.ro = (image_offset(d.rmap, a.r_plain, a.dRin, n) + u.off + c0) * 4;
        r.ox = u.last_x ? 0 : d.ldr * 4;
        r.oy = u.last_y ? 0 : (d.wo >> 1) * d.ldr * 4;
    }
    return r;
}
// the record of the row that lane `src` owns, at this lane's channel quad qd
template <int RESK>
__device__ __forceinline__ PwRow pw_row_from(const PwRow& own, int src, int qd) {
    PwRow r = {0, 0, 0, 0, 0.f, 0.f};
    r.yo = __shfl(own.yo, src) + qd * 16;
    if constexpr (RESK != 0) r.ro = __shfl(own.ro, src) + qd * 16;
    if constexpr (RESK == 2) {
        r.ox = __shfl(own.ox, src); r.oy = __shfl(own.oy, src);
        r.lx1 = __shfl(own.lx1, src); r.ly1 = __shfl(own.ly1, src);
    }
    return r;
}
// epi_value in these kernels' branch-free form: the activation is ReLU or none (floor_ = 0 / -inf: one select) and the residual's
// place a select too (RESK 1: r00 before the activation when res_before, behind it otherwise), so that a row is straight-line code.
// RESK 2: r00 r01 / r10 r11 are the four corners.  The ReLU mask of the masked launches follows at the site.
template <int RESK>
__device__ __forceinline__ float pw_value(float acc, float sc, float sh, const float& r00, const float& r01, const float& r10, const float& r11,
                                          float lx1, float ly1, bool res_before, float floor_) {      // (corners by reference: only RESK's are read)
#pragma clang fp contract(off)
    float tt = __builtin_fmaf(acc, sc, sh);
    if constexpr (RESK == 1) tt += res_before ? r00 : 0.f;
    if constexpr (RESK == 2) tt = up2_res_add(tt, r00, r01, r10, r11, lx1, ly1);
    tt = tt > floor_ ? tt : floor_;
    if constexpr (RESK == 1) tt += res_before ? 0.f : r00;
    return tt;
}
__device__ __forceinline__ float pw_value(float acc, float sc, float sh, float floor_) { return pw_value<0>(acc, sc, sh, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false, floor_); }

}  // namespace egrc
