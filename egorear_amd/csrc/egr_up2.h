// Bilinear x2, align_corners=True: the ONE statement of the index / weight / interpolation arithmetic that a kernel evaluating
// ReLU(up2(x)) on the fly must share with upsample2x_kernel (egr_pointwise.hip) to be bit-identical to it.
// ATen's area_pixel_compute_source_index(align_corners=True): src = dst * (in - 1) / (out - 1) in fp32, i0 = (int)src,
// i1 = min(i0 + 1, in - 1), l1 = src - i0 clamped to [0, 1], l0 = 1 - l1.
// The operation order below is the one the compiler gives upsample2x_kernel (its contractions written out, none left to it):
//   scale   (float)(in - 1) / (float)(out - 1)                          correctly rounded division
//   i0      (int)(scale * dst)                                          the ROUNDED product, truncated
//   l1      clamp(fma(scale, dst, -i0))                                 the UNROUNDED product minus i0
//   value   fma(ly0, fma(lx0, v00, lx1 * v01), ly1 * fma(lx0, v10, lx1 * v11)),  then  t < 0 ? 0 : t
#pragma once
#include "egr_common.h"

namespace egr_up2 {

__device__ __forceinline__ float scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

struct Axis {
    int i0, i1;        // the two source indices
    float l0, l1;      // their weights
};

// output coordinate o of an axis with `in` source samples
__device__ __forceinline__ Axis axis(float s, int o, int in) {
#pragma clang fp contract(off)
    const float fo = (float)o;
    const float f = s * fo;
    Axis a;
    a.i0 = (int)f;
    a.i1 = a.i0 + 1 < in - 1 ? a.i0 + 1 : in - 1;
    a.l1 = fminf(fmaxf(__builtin_fmaf(s, fo, -(float)a.i0), 0.f), 1.f);
    a.l0 = 1.f - a.l1;
    return a;
}

// first source index of output coordinate o (the i0 of axis(), alone)
__device__ __forceinline__ int first_index(float s, int o) {
#pragma clang fp contract(off)
    return (int)(s * (float)o);
}

// one value from its four corners (v00 v01 / v10 v11 = row i0, row i1), ReLU applied as upsample2x_kernel(relu = 1) applies it
__device__ __forceinline__ float lerp_relu(float v00, float v01, float v10, float v11, float lx0, float lx1, float ly0, float ly1) {
#pragma clang fp contract(off)
    const float top = __builtin_fmaf(lx0, v00, lx1 * v01);
    const float bot = __builtin_fmaf(lx0, v10, lx1 * v11);
    const float t = __builtin_fmaf(ly0, top, ly1 * bot);
    return t < 0.f ? 0.f : t;
}

}  // namespace egr_up2
