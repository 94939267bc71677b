/*
 * egorear_hip.h — C ABI of the MI355X (gfx950) kernels for EgoRear's multi-view
 * inference hot path (heatmap encoder -> MVFEx/JQA refinement -> 2D-to-3D lifting).
 *
 * The reference is pure Python on PyTorch; the boundary it offers for native code is
 * its operator level.  Each entry point below names the reference
 * interface it replaces (paths relative to /root/reference/pose_estimation/).  The
 * one native op the reference itself binds is mmcv's
 * MultiScaleDeformableAttnFunction (models/utils/deform_attn.py:9,155-162); here it is
 * egr_msda_gather_f32 + egr_conv2d_nhwc_f32 (sample-then-project form).
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless noted;
 *   - activations are fp32, channels-last ("NHWC"): pixel-major, channel-minor, with an
 *     explicit pixel stride `ld*` (floats) so that channel slices of a wider buffer can
 *     be read/written in place (virtual concat);
 *   - image index n of a batch maps to memory as
 *         base + (n % n_inner) * stride_inner + (n / n_inner) * stride_outer
 *     which covers plain batches (n_inner = N) and view-major <-> batch-major
 *     re-orderings at the boundary;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous, nothing
 *     synchronises, allocates or frees, so every call is hipGraph-capturable;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     EGR_E* code for arguments the kernels do not support (nothing is launched then).
 */
#ifndef EGOREAR_HIP_H
#define EGOREAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGR_EINVAL (-1)   /* unsupported shape / alignment */
#define EGR_ENULL (-2)    /* required pointer is NULL */
#define EGR_EWORKSPACE (-3) /* workspace too small */

enum { EGR_ACT_NONE = 0, EGR_ACT_RELU = 1, EGR_ACT_GELU = 2 };           /* GELU = exact erf form */
enum { EGR_RES_NONE = 0, EGR_RES_BEFORE_ACT = 1, EGR_RES_AFTER_ACT = 2,
       EGR_RES_UP2_BEFORE_ACT = 3 /* res is a (ho/2, wo/2) tensor: its bilinear x2 upsampling (align_corners=True) is added before the activation */ };

/* image-index -> offset mapping (floats) */
typedef struct {
    int32_t n_inner;
    int64_t stride_inner;
    int64_t stride_outer;
} egr_nmap;

/*
 * Convolution / linear layer as one implicit GEMM on fp32 MFMA.
 *   y[n,ho,wo,co] = act( acc * scale[co] + shift[co] * (rowscale ? rowscale[m] : 1) (+ res) )
 *   acc = sum_{kh,kw,ci} x[n, ho*stride-pad+kh, wo*stride-pad+kw, ci] * w[co, (ci/32, kh, kw, ci%32)]
 * (weights packed [round_up(cout,32)][cin/32][kh*kw][32]: all taps of one 32-channel chunk are adjacent in K)
 * with m = (n*ho_total + ho)*wo_total + wo.  A Linear layer is the case h=w=kh=kw=1, n=rows.
 * Replaces nn.Conv2d(+BatchNorm2d eval)(+ReLU)(+residual) of models/backbones/resnet.py:43-137
 * and of the conv stacks in models/estimator/egoposeformer_heatmap_mvf_ex.py:101-126,522-584 /
 * egoposeformer_mvf_ex.py:144,229-239, and nn.Linear(+ReLU/GELU) of models/utils/transformer.py:8-93,
 * deform_attn.py:60-63, egoposeformer_mvf_ex.py:156-162,241-262.
 */
typedef struct {
    int32_t n, h, w, cin;        /* input: n images of h x w pixels, cin channels (cin % 32 == 0) */
    int32_t cout;                /* true output channels; w holds round_up(cout,32) rows, zero padded */
    int32_t kh, kw, stride, pad;
    int32_t ho, wo;
    int32_t ldx, ldy, ldr;       /* pixel strides (floats) of x, y, res */
    egr_nmap xmap, ymap, rmap;   /* per-image placement of x, y, res */
    int32_t act;                 /* EGR_ACT_* */
    int32_t res_mode;            /* EGR_RES_* */
    int32_t out_nchw;            /* 1: y is written channel-major: ymap(n) + co*ho*wo + pix */
    int32_t split_k;             /* >1: partial sums go through `workspace` (groups * split_k * M * round_up(cout,32) floats) */
    /* Grouped launch: `groups` independent problems of identical shape (e.g. the two stereo estimators, the four
     * per-view refiners — same architecture, own weights) in one launch.  Group g uses x + g*gx, w + g*gw,
     * scale/shift + g*gp, res + g*gr, rowscale + g*grs, rowmask + g*grm, y + g*gy (strides in elements; 0 = shared). */
    int32_t groups;
    int64_t gx, gw, gp, gy, gr, grs, grm;
    /* Transposed (data-gradient) mode, first brick of the training row: with `transposed` = 1 the
     * launch computes dx = conv_transpose(dy, W): x is dy (n, h, w, cin = forward cout), y is dx (n, ho, wo, cout = forward
     * cin) — ho/wo are given, not derived — stride/pad/kh/kw are the FORWARD conv's, and w is the forward weight packed with
     * its in/out channels swapped ([cin_fwd_pad][cout_fwd/32][kh*kw][32]).  Row m = (n, hi, wi) gathers
     * dy[n, (hi+pad-kh)/stride, (wi+pad-kw)/stride, :] for the taps where the division is exact and in range. */
    int32_t transposed;
    /* Weight operand format.  EGR_W_F32 (0): w is the packed fp32 matrix described above, multiplied on the fp32 matrix
     * cores.  EGR_W_BF16X3 (1): w points to the image egr_pack_w6_f32 made of that matrix — every weight as the exact sum
     * of three bf16 numbers, in MFMA-fragment order — and the launch runs on the bf16 matrix cores: the activations are
     * split the same way on the fly and the six partial products of order <= 2 are accumulated in fp32 (the dropped
     * ones are below 2^-25 relative: the result is as close to the exact sum as an fp32 fma chain).
     * gw is then in bf16 elements (egr_w6_elems per group). */
    int32_t w_format;
} egr_conv_desc;
enum { EGR_W_F32 = 0, EGR_W_BF16X3 = 1,
       EGR_W_FORCE = 2 /* egr_conv2d_wgrad_f32 only: with EGR_W_BF16X3, take the split kernel whatever the problem size (tests) */,
       EGR_W_F16X2 = 4 /* egr_conv2d_nhwc_ex_f32 only: w is the image egr_pack_wh2_f32 made (two fp16 planes per weight) */,
       /* With EGR_W_F16X2 (egr_conv2d_nhwc_ex_f32 / egr_conv_plan; EGR_EINVAL with any other format): the opt-in fast policy (DESIGN.md
        * §5k).  w is the same F16X2 image; where a one-product kernel exists - the forward launches of the role-split route - both
        * operands are multiplied as their HIGH planes only, f16(x 2^e) f16(w 2^k), one matrix product instead of three: fp16-rounded
        * operands (relative 2^-11 each), fp32 accumulation.  Every other launch treats the bit as absent. */
       EGR_W_F16X1 = 8,
       /* With EGR_W_F16X2 | EGR_W_F16X1 only (EGR_EINVAL otherwise): the half-precision TRAINING policy.  The training
        * launches of the role-split route - statistics epilogue, masked and plain stride-1 data gradients - take their one-product form
        * too.  Every other launch treats the bit as absent.  egr_conv2d_wgrad_ex_f32 does not read it: there EGR_W_F16X1 beside
        * EGR_W_BF16X3 | EGR_W_F16X2 asks for the one-product split kernels. */
       EGR_W_F16X1T = 16 };

/* Split a packed fp32 weight matrix w (groups, npad, k) — npad = round_up(cout, 32), k = kh*kw*cin, k % 32 == 0 — into
 * the EGR_W_BF16X3 image: per group egr_w6_elems(npad, k) bf16 elements laid out
 * [round_up(npad/32, 4) column fragments][k/32 chunks][2 k16 steps][3 planes hi, mid, lo][64 lanes][8 bf16],
 * lane l of a fragment holding w[col = 32*frag + (l & 31)][k = 32*chunk + 16*step + 8*(l >> 5) + j], j = 0..7.
 * hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid), round to nearest even: hi + mid + lo == w exactly
 * (fragments beyond npad/32 are zero).  img must be 16-byte aligned. */
int64_t egr_w6_elems(int32_t npad, int32_t k);
int egr_pack_w6_f32(const float* w, int32_t npad, int32_t k, int32_t groups, void* img, void* stream);

/* The same for many matrices in one launch.  jobs: DEVICE array of `count` records sorted by first_block, record i covering the
 * workgroups [first_block_i, first_block_i + groups_i * round_up(npad_i/32, 4) * k_i/32); total_blocks = the end of the last one. */
typedef struct {
    const float* w;
    void* img;
    int32_t npad, k, groups, reserved;
    int64_t first_block;
} egr_w6_job;
int egr_pack_w6_many_f32(const egr_w6_job* jobs, int32_t count, int64_t total_blocks, void* stream);

/* Split a packed fp32 weight matrix w (groups, npad, k) into the EGR_W_F16X2 image: every weight, multiplied by the power of two
 * s[co] that puts the largest magnitude of its row (output channel) into [2^14, 2^15), as h = f16(w s) and l = f16(w s - h) (round to
 * nearest even; h + l carries 22 significant bits of w, fp16 subnormals included).  Layout per group (egr_wh2_elems(npad, k) 16-bit
 * elements): [round_up(npad/32, 4) column fragments][k/32 chunks][2 k16 steps][2 planes h, l][64 lanes][8 fp16], lane / k mapping as in
 * egr_pack_w6_f32.  descale (groups, npad) receives 1 / s[co] (exact powers of two, clamped to 2^+-60), which the launch multiplies
 * back into its accumulators.  Replaces nothing in the reference: it is the operand format of the launches that replace
 * nn.Conv2d / nn.Linear (see egr_conv2d_nhwc_f32) on the fp16 matrix cores. */
int64_t egr_wh2_elems(int32_t npad, int32_t k);
int egr_pack_wh2_f32(const float* w, int32_t npad, int32_t k, int32_t groups, void* img, float* descale, void* stream);
/* The same for every job of a device-resident table in two launches (the training step re-splits all its weight operands after every
 * parameter update): first_rblock / first_pblock = running counts of ceil(groups npad / 4) and groups round_up(npad/32, 4) (k/32)
 * over the jobs before this one; total_* their sums. */
typedef struct {
    const float* w;
    void* img;
    float* descale;
    int32_t npad, k, groups, reserved;
    int64_t first_rblock, first_pblock;
} egr_wh2_job;
int egr_pack_wh2_many_f32(const egr_wh2_job* jobs, int32_t count, int64_t total_rblocks, int64_t total_pblocks, void* stream);

int egr_conv2d_nhwc_f32(const egr_conv_desc* d, const float* x, const float* w,
                        const float* scale /* per co, NULL = 1 */, const float* shift /* per co, NULL = 0 */,
                        const float* res /* NULL unless res_mode */, const float* rowscale /* per m, NULL = 1 */,
                        const uint8_t* rowmask /* per m, NULL = keep; 0 -> row written as 0 */,
                        float* y, float* workspace, size_t workspace_floats, void* stream);

/* egr_conv2d_nhwc_f32 with the side operands of the fp16 scheme.  EGR_W_F16X2 launches multiply on
 * v_mfma_f32_32x32x16_f16: both operands as two fp16 planes of the value times an exact power of two, the three products
 * (l,h) (h,l) (h,h) accumulated in fp32, the accumulators multiplied by the inverse powers before the epilogue.  Measured against
 * fp64 the result is as close to the exact sum as an fp32 fma chain (tools/proto/f16x3_accuracy.hip).  The pre-scale of the
 * activations comes from a record of their largest magnitude that the PRODUCING launch left behind:
 *   amax_out  (any w_format; NULL = off) 64 uint32 slots, zero before the launch: the launch folds max |y| over everything it
 *             stores into them (atomic max on the float bits; the record is the maximum over the 64 slots);
 *   amax_in   (EGR_W_F16X2) the record of x: any upper bound of max |x| serves (a tensor derived from x by max-pooling or bilinear
 *             interpolation inherits x's record); the launch scales x by 2^k with max |x| 2^k in [2^14, 2^15), k clamped to +-60;
 *   w_descale (EGR_W_F16X2) the per-channel descale egr_pack_wh2_f32 wrote ((groups,) round_up(cout, 32) floats, group stride gp).
 * w: the fp32 matrix, the egr_pack_w6_f32 image or the egr_pack_wh2_f32 image as w_format says (gw in 16-bit elements for both
 * images).  EGR_W_F16X2 covers forward, transposed (data-gradient) and masked launches alike (the training step runs all three on
 * it); amax_out does not go with out_nchw. */
typedef struct {
    const float* w_descale;
    const uint32_t* amax_in;
    uint32_t* amax_out;
    /* Train-mode BatchNorm behind the conv (nn.BatchNorm2d on batch statistics, models/backbones/resnet.py:43-137 in train()): the
     * launch also leaves, per M tile and output channel, the sum / sum of squares (double) and min / max (float) of what it stores -
     * the slabs egr_bn_stats_f32's first pass would produce by reading y again; egr_bn_finalize_f32 (egorear_train.h) consumes them.
     * bn_partials: 16-byte aligned, bn_capacity doubles; layout [groups][tiles][2][cout] doubles followed by the same shape in floats,
     * `tiles` = *bn_tiles_out (host int, written before the launch is enqueued: the launch's M tiles per group).  Raw NHWC output
     * only (no activation / residual / row modifiers, cout % 64 == 0); EGR_EINVAL otherwise, EGR_EWORKSPACE when the slabs do not fit -
     * the caller then runs the statistics pass. */
    double* bn_partials;
    int32_t* bn_tiles_out;
    int64_t bn_capacity;
    /* Input mode.  EGR_IN_PLAIN (0): x is the operand.  EGR_IN_UP2_RELU (1): x is a HALF-RESOLUTION tensor - d->h / 2 x d->w / 2
     * pixels per image, pixel pitch ldx, images by xmap - and the operand is ReLU(bilinear x2(x)), align_corners=True, evaluated as
     * the launch loads it: bit-identical to egr_upsample2x_nhwc_f32(relu = 1) followed by the plain launch, without the
     * full-resolution tensor in between.  d describes the conv on the up-sampled image (h = ho, w = wo).  amax_in is the record of
     * x: it bounds the interpolated operand.  in_up2_out (optional, 16-byte aligned): the launch also WRITES the operand, dense
     * ((groups,) n, h, w, cin), for consumers that read it from memory - one pass over it instead of the up-sampling launch's write
     * and this launch's read.
     * Implemented by the streaming route alone: 1x1 / stride 1 / pad 0, cin 128, EGR_W_F16X2 (the one-product bits change nothing: that route has no such form), NHWC
     * output, no residual / mask / row modifiers / statistics, w % 32 == 0 (a wave's 32 pixels lie in one row), enough rows for that
     * route.  Every other call - other kernel sizes and strides, odd geometry, EGR_W_F32 / EGR_W_BF16X3, transposed, masked and
     * statistics launches, out_nchw - returns EGR_EINVAL, from egr_conv_plan too, and launches nothing. */
    int32_t in_mode;
    float* in_up2_out;
} egr_conv_aux;
enum { EGR_IN_PLAIN = 0, EGR_IN_UP2_RELU = 1 };
int egr_conv2d_nhwc_ex_f32(const egr_conv_desc* d, const float* x, const void* w, const float* scale, const float* shift,
                           const float* res, const float* rowscale, const uint8_t* rowmask, float* y, float* workspace,
                           size_t workspace_floats, const egr_conv_aux* aux /* NULL = egr_conv2d_nhwc_f32 */, void* stream);

/* Two 1x1 / stride-1 convolutions back to back in ONE launch (fp16 scheme, round 5):
 *     y = act2( W2 . act1( W1 . x + shift1 ) + shift2 [+ res] )
 * with the cmid-channel intermediate kept in the accumulator registers of the lane that owns the pixel (never written to memory) -
 * it is split into its two fp16 planes under a PER-PIXEL power-of-two scale and fed back to the matrix cores as the second product's
 * operand.  Replaces the pairs nn.Conv2d(1x1)+ReLU -> nn.Conv2d(1x1)[+ReLU] of the path whose intermediate used to round-trip
 * through HBM: EfficientFPN's lateral conv -> fuse conv (models/backbones/resnet.py:96-110, 127-133; the fuse conv's up-sampled half
 * enters as res with EGR_RES_UP2_BEFORE_ACT) and HeatmapMVF.frame_feat_refined_proj_layers
 * (models/estimator/egoposeformer_heatmap_mvf_ex.py:553-563, 715).
 * d: the chain described as ONE 1x1 conv cin -> cout (n, h = ho, w = wo, ldx / ldy / ldr, the three maps, act = act2, res_mode,
 *    groups with gx / gy / gr / gp, gw = 16-bit elements between the groups' W1 images; kh = kw = stride = 1, pad = 0,
 *    w_format = EGR_W_F16X2); cin 64 or 128 with chain->cmid 128 (both weight images stay in LDS), or cin 256 with chain->cmid 256 and
 *    no residual (the heat-map heads' Conv2d(256, 256, 1) + ReLU -> [Upsample ->] Conv2d(256, 128, 1),
 *    egoposeformer_heatmap_mvf_ex.py:101-126, 570-584: both images are STREAMED through a four-slot LDS ring, one 8-KB chunk per k16
 *    step, and the intermediate is produced / consumed in two halves of 128 channels, each under its own per-pixel scale);
 *    cout <= 128 (cout % 4 == 0).
 * w1 / aux->w_descale: egr_pack_wh2_f32 image and descale of the first conv (cmid x cin; descale group stride chain->gp1);
 * aux->amax_in: abs-max record of x; aux->amax_out: record of y (may be NULL); shift2 / chain->w2_descale: (groups,) 128 floats,
 * group stride d->gp.  EGR_EINVAL for any other shape - the caller then runs the two launches of egr_conv2d_nhwc_ex_f32. */
typedef struct {
    const void* w2;            /* egr_pack_wh2_f32 image of the second conv (round_up(cout, 32) padded to 128 rows x cmid) */
    const float* w2_descale;
    const float* shift1;       /* bias of the first conv, (groups,) cmid floats, group stride gp1; NULL = 0 */
    int32_t cmid, act1;        /* 128 (256 with cin 256); EGR_ACT_NONE | EGR_ACT_RELU */
    int64_t gw2, gp1;          /* group strides: 16-bit elements of w2; floats of shift1 and of aux->w_descale */
} egr_chain_aux;
int egr_conv1x1_chain_f32(const egr_conv_desc* d, const float* x, const void* w1, const float* shift2, const float* res, float* y,
                          const egr_conv_aux* aux, const egr_chain_aux* chain, void* stream);

/* Data gradient behind a ReLU (training row): the conv of `d` (normally in transposed mode) with y = (conv [+ res]) * [mask > 0],
 * mask laid out exactly like y (the forward activation the ReLU produced).  Fuses torch's threshold_backward into the
 * data-gradient launch of the layer above.  No scale / shift / activation; res (may be NULL) is added before the mask. */
int egr_conv2d_masked_f32(const egr_conv_desc* d, const float* x, const float* w, const float* res, const float* mask, float* y,
                          float* workspace, size_t workspace_floats, void* stream);
/* ... with the side operands of the fp16 scheme (egr_conv_aux, see egr_conv2d_nhwc_ex_f32): the data-gradient launches of the
 * training step on the fp16 matrix cores, max |dx| recorded for the launch that consumes dx. */
int egr_conv2d_masked_ex_f32(const egr_conv_desc* d, const float* x, const void* w, const float* res, const float* mask, float* y,
                             float* workspace, size_t workspace_floats, const egr_conv_aux* aux, void* stream);

/* What a launch of egr_conv2d_nhwc[_ex]_f32 / egr_conv2d_masked[_ex]_f32 will do, decided on the host before anything is launched
 * (DESIGN.md §5j).  The route values are the codes egr_conv_last_kernel() reports. */
typedef enum {
    EGR_ROUTE_F32_TILED = 0,     /* fp32 matrix cores, one BM x BN tile per workgroup (EGR_W_F32) */
    EGR_ROUTE_SPLIT_TILED = 1,   /* the same tiles on the 16-bit matrix cores (EGR_W_BF16X3 / EGR_W_F16X2), persistent for short K */
    EGR_ROUTE_TAP = 2,           /* 3x3 / stride 1 / pad 1, tiles of whole image rows: the taps share one staged halo */
    EGR_ROUTE_TAP2 = 3,          /* 3x3 / stride 2 / pad 1 on even images: taps shared by input parity class (env EGR_CONV_TAP2=0: off) */
    EGR_ROUTE_STREAM_1X1 = 4,    /* 1x1, cin 64 / 128, many rows: weights stationary in LDS, activations streamed (env EGR_CONV_PW=0: off) */
    EGR_ROUTE_SMALL_F32 = 5,     /* small fp32 1x1 / stride 1: one 32 x 32 tile per workgroup, K split over its four waves, operands read
                                  * straight from global memory (env EGR_CONV_SMALL=0: off); sums differ from route 0's in the last bits */
    EGR_ROUTE_TAPX = 6           /* fp16 scheme, 3x3 and wide 1x1: role-split persistent workgroups (egr_conv_set_tapx) */
} egr_conv_route;
typedef struct {
    int32_t route;               /* egr_conv_route */
    int32_t bm, bn;              /* tile rows x columns (STREAM_1X1: 32 rows per wave step, NCF * 32 columns) */
    /* which kernel of the route where the tile does not say it all:
     *   F32_TILED / SPLIT_TILED  the tile configuration (egr_conv_force_config numbering)
     *   STREAM_1X1               100 KS + 10 NCF + RESK  (KS = cin / 16, NCF = 32-column fragments per workgroup, RESK 0 no residual /
     *                            1 residual / 2 residual upsampled on the fly)
     *                            + 1000: egr_conv_aux.in_mode = EGR_IN_UP2_RELU (the operand up-sampled as it is loaded),
     *                            + 2000: the same with the operand written out (in_up2_out)
     *   TAPX                     100 T + 10 R + cfg  (T 0 forward / 1 statistics epilogue / 2 masked data gradient, R 1 with residual,
     *                            cfg = the kernel's (tile, wave tile, stride) configuration 0, 1, 3 .. 7); + 1000: the one-product
     *                            form of a forward variant (EGR_W_F16X1) or of a training / data-gradient one (EGR_W_F16X1T)
     *   others                   0 */
    int32_t variant;
    int32_t planes;              /* 16-bit planes multiplied per operand: 2 (EGR_W_F16X2), 3 (EGR_W_BF16X3), 0 (fp32); 1: a one-product
                                  * launch (EGR_W_F16X1 on a TAPX forward variant, EGR_W_F16X1T on the others) */
    int32_t tiles_m, tiles_n;    /* tiles per group */
    int32_t grid_x, grid_y, grid_z, block;     /* the main launch */
    int32_t split_k, ktiles_per_split;        /* K slices (1: none) of ktiles_per_split 32-deep chunks, none empty */
    int32_t persistent;          /* workgroups walk several tiles (grid_x < tiles) */
    int32_t cls_mode;            /* stride-2 data gradient as four output-parity classes (grid_y = 4) */
    int32_t fused_reduce;        /* split_k > 1: the fused reduction was requested (egr_conv_set_splitk_fused) and the tiles fit a counter region */
    int32_t reduce_pass;         /* split_k > 1: a reduction launch follows (also taken when fused_reduce finds no free counter region) */
    int32_t bn_slabs;            /* egr_conv_aux.bn_partials: the slab count reported through bn_tiles_out (= tiles_m), else 0 */
} egr_conv_plan_t;
/* The plan of the launch the four entry points above would make for these arguments, without launching: same checks, same return
 * code as the launch would give before its first kernel (EGR_E*, 0 = `out` is filled).  No data pointer is dereferenced (only
 * NULL-ness and alignment count; `aux` is host memory and is read, nothing is written through aux->bn_tiles_out), no device is touched.
 * mask = NULL: egr_conv2d_nhwc_ex_f32, else egr_conv2d_masked_ex_f32 (scale / shift / rowscale / rowmask NULL). */
int egr_conv_plan(const egr_conv_desc* d, const float* x, const void* w, const float* scale, const float* shift,
                  const float* res, const float* rowscale, const uint8_t* rowmask, const float* mask, const float* y,
                  const float* workspace, size_t workspace_floats, const egr_conv_aux* aux, egr_conv_plan_t* out);

/* Weight (and bias) gradient of the conv / linear layer described by `d` (forward geometry; d->groups same-shape problems
 * in one launch: x + g*gx, dy + g*gy, dw + g*gw, db + g*gp), the weight-side half of the training row: dw[co][(ci/32, kh, kw, ci%32)] (+)= sum over output pixels of dy[m][co] * im2col(x)[m][k],
 * db[co] (+)= sum_m dy[m][co] (db may be NULL).  dw is in the packed weight layout of egr_conv2d_nhwc_f32.  The pixels are
 * split over workgroups; partial tiles go through `workspace` and are summed in fixed order (deterministic).
 * Replaces autograd of nn.Conv2d / nn.Linear for config 5 (pl_wrappers/egoposeformer/pose_3d_mvf_ex.py:117-153). */
/* d->w_format & EGR_W_BF16X3: large problems (>= 1024 pixels and >= 4 GFLOP) run on the bf16 matrix cores with both operands
 * split exactly into three bf16 on the fly; the result class is the fp32 kernel's. */
int egr_conv2d_wgrad_f32(const egr_conv_desc* d, const float* x, const float* dy, float* dw, float* db,
                         float* workspace, size_t workspace_floats, int32_t accumulate, void* stream);
/* ... in the fp16 scheme when d->w_format carries EGR_W_F16X2 beside EGR_W_BF16X3 [| EGR_W_FORCE]: the split launches
 * then take both operands as two fp16 planes of the value times a power of two from its abs-max record (amax_x / amax_dy: 64 slots
 * each, as egr_conv_aux.amax_in) - three matrix products per fp32 product instead of six; the accumulators are scaled back when the
 * partial tiles are written.  Launches below the split threshold ignore the records (fp32 matrix cores).
 * EGR_W_F16X1 on top of that (EGR_EINVAL without EGR_W_F16X2): the split launches stage the HIGH plane of both operands only,
 * f16(dy 2^e) f16(x 2^k), and issue ONE product (outside the parity contract).  Same records, same slabs and split
 * count, same bias gradient (a sum of fp32 dy: bit-identical to the three-product launch's). */
int egr_conv2d_wgrad_ex_f32(const egr_conv_desc* d, const float* x, const float* dy, float* dw, float* db, float* workspace,
                            size_t workspace_floats, int32_t accumulate, const uint32_t* amax_x, const uint32_t* amax_dy, void* stream);
/* diagnostic (tests): 1 when the last weight-gradient call launched a fp16-scheme kernel */
int egr_wgrad_last_h2(void);
/* diagnostic (tests): 16-bit planes per operand of the last weight-gradient call's main launch - 1 (EGR_W_F16X1), 2 (fp16 scheme), 3 (bf16
 * scheme); 0: a fp32 kernel */
int egr_wgrad_last_planes(void);
/* diagnostic (tests): the kernel the last egr_conv2d_wgrad_f32 call launched - 0 fp32 MFMA, 1 split-bf16 generic,
 * 2 / 3 split-bf16 3x3 stride-1 tap-sharing (64 channels x 2 input chunks / 128 x 1), 4 the small 1x1 kernel (fp32 path, 1x1 / stride 1,
 * rows x groups <= 8192, at most 256 tiles of 32 x 32: weight and bias gradient in ONE launch, no slabs; env EGR_WGRAD_SMALL=0
 * turns it off). */
int egr_wgrad_last_kernel(void);

/* Tuning knob for measurements: force the tile configuration of egr_conv2d_nhwc_f32
 * (-1 auto, 0 128x128, 1 256x64, 2 64x64, 3 128x32, 4 128x64).  Process-wide; results do not depend on it. */
int egr_conv_force_config(int cfg);
/* diagnostic (tests): the route (egr_conv_route) of the last plan that egr_conv2d_nhwc[_ex]_f32 / egr_conv2d_masked[_ex]_f32
 * launched.  egr_conv_set_tap(0) disables routes 2-4 and 6.  The rules that pick a route are the plan_* functions of
 * csrc/egr_conv.hip / egr_conv_tapx.hip, pinned case by case in tests/golden/conv_plan_cases.json.
 * Environment (read once at load; all integers): EGR_CONV_TAP, EGR_CONV_TAP2, EGR_CONV_TAP64, EGR_CONV_PW, EGR_CONV_PW_MIN_ROWS,
 * EGR_CONV_PW_BLOCKS, EGR_CONV_SMALL, EGR_CONV_SMALL_K, EGR_CONV_SMALL_TILES, EGR_CONV_SMALL_ROWS, EGR_CONV_PERSIST,
 * EGR_CONV_PERSIST_KTILES, EGR_SPLITK_FUSED, EGR_SPLITK_MID_KT (automatic split-K of fp32 launches with 128 .. 511 workgroups: from
 * this many 32-deep chunks, default 16, 0 = only from 64), EGR_SPLITK_TARGET (workgroups an automatic split aims at, default 1024),
 * EGR_CONV_TAPX, EGR_CONV_TAPX_MIN_TILES, EGR_CONV_TAPX_BLOCKS, EGR_CONV_TAPX_PW, EGR_CONV_TAPX_TPW, EGR_CONV_TAPX_TRAIN,
 * EGR_CONV_TAPX_FN - defaults and meanings: load_conv_knobs in csrc/egr_conv.hip. */
int egr_conv_last_kernel(void);
/* diagnostic / test knob: 1 = split-K launches run the reduction + epilogue in the last-arriving K slice of each tile (arrival
 * counters, agent-scope slab accesses) instead of a second kernel (splitk_reduce_kernel).  Both sum the slices in slice order.
 * Default 0 (env EGR_SPLITK_FUSED): the fused form saves the launch but measured slower, see DESIGN.md §5d.  The counters are
 * one region per `workspace` pointer (launches that share a workspace cannot overlap anyway; two engine lanes own one each, also
 * when their graphs were captured on the same stream), 64 workspaces per process at most - the 65th takes the second pass. */
int egr_conv_set_splitk_fused(int on);
/* diagnostic / test knob: 0 = 3x3 stride-1 split launches stay on the generic split kernel (default 1, env EGR_CONV_TAP); 3 = the
 * tap-sharing kernels without the 64-row tile that launches below 256 tiles of 128 x 64 take in the fp16 scheme (batch 1: twice the
 * workgroups; env EGR_CONV_TAP64=0).  Same results either way. */
int egr_conv_set_tap(int on);
/* Test / tuning knob of the fp16 scheme's 3x3 / pad 1 forward launches (stride 1 with 64-channel-multiple outputs, stride 2 with
 * 256-channel-multiple outputs; nn.Conv2d 3x3 of models/backbones/resnet.py:43-74 and of the heads / refiners in
 * models/estimator/egoposeformer_heatmap_mvf_ex.py:101-126, 525-532, 570-584): launches with at least `min_tiles` output tiles over
 * all groups run on role-split persistent workgroups - four multiplying waves + four waves that load, split and run the previous
 * tile's epilogue under the current tile's K loop, `blocks` workgroups (one per CU) - egr_conv_last_kernel() = 6.  on = 0 keeps them
 * on the tap-sharing kernels (2 / 3); on = 2 / 3 force the 128 x 32 / 128 x 64 wave tile wherever that variant exists (1: chosen by
 * shape).  Negative values leave a setting unchanged; defaults 1, 256, 256 (env EGR_CONV_TAPX, EGR_CONV_TAPX_MIN_TILES,
 * EGR_CONV_TAPX_BLOCKS, EGR_CONV_TAPX_FN).  Process-wide; results do not depend on it (same products, same summation order).
 * Training launches take the same kernel where it measured faster (env EGR_CONV_TAPX_TRAIN=0: never): a 3x3 conv with the
 * statistics epilogue (egr_conv_aux.bn_partials; slabs = M tiles of the tile height chosen, 256 or 128 rows) and the stride-1 data
 * gradient (transposed, plain or through egr_conv2d_masked_f32) - from four tiles per CU, masked launches for 64-channel outputs only. */
int egr_conv_set_tapx(int32_t on, int32_t min_tiles, int32_t blocks);
/* Tuning / test knob of the persistent split-bf16 launches (short-K layers: a workgroup walks several tiles and requests the next
 * tile's operands under the current tile's stores): `slots` = resident workgroups a launch is sized for (0: never persistent;
 * default 512 = 2 per CU), `max_ktiles` = largest K in 32-deep chunks that takes them (default 4).  Negative: unchanged.
 * Process-wide; results do not depend on it. */
int egr_conv_set_persist(int slots, int max_ktiles);

/* Tail of a heat-map head in one pass: Upsample(x2, bilinear, align_corners=True) + ReLU, then the final 1x1 conv
 * (cin <= 128 -> cout <= 16, with bias) written as channel-major planes: lo (n, h, w, cin) NHWC, all groups' images back to back;
 * wgt (groups, cout, cin) plain row-major; image i of group g goes to planes + g*gy + nmap(i).  The cin-channel tensor at the
 * doubled resolution is never materialised.  Replaces `nn.Upsample -> ... -> ReLU -> Conv2d(128, 15, 1)` of
 * egoposeformer_heatmap_mvf_ex.py:101-126 (indices 6-9) and :570-584 (indices 4-7); 2h % 8 == 0, 2w % 32 == 0, cin % 16 == 0. */
int egr_up2_relu_head_f32(const float* lo, int32_t n, int32_t h, int32_t w, int32_t cin, const float* wgt, const float* bias,
                          int32_t cout, float* planes, int32_t n_inner, int64_t stride_inner, int64_t stride_outer,
                          int32_t groups, int64_t gy, void* stream);
/* Which kernel egr_up2_relu_head_f32 launches for 128 input channels and >= 1024 tiles (round 5): 1 (default; EGR_HEAD_PERSIST) =
 * persistent eight-wave workgroups that request the next tile's source pixels under the current tile's arithmetic, 0 = one
 * workgroup per tile; bit-identical results.  on < 0 only queries.  Returns the previous setting. */
int egr_head_set_persist(int on);

/* Diagnostic only (tools/conv_stamps.py): when `buf` is non-NULL every conv workgroup writes 8 x uint64 — s_memtime at
 * [0] start, [1] row decode done, [2] first chunk landed, [3] K loop done, [4] accumulators staged, [5] stores issued, and
 * [6] its physical placement (XCC id << 16 | HW_ID) — to buf[8 * workgroup].  NULL (the default) disables it. */
int egr_conv_debug_stamps(unsigned long long* buf);

/* ResNet stem: conv 7x7 stride 2 pad 3 (3 -> 64) + BatchNorm(eval) + ReLU, NCHW fp32 input
 * (h, w multiples of 64) -> NHWC output (n, h/2, w/2, 64).  w: [64][148] rows = (ci,kh,kw), last col 0.
 * Replaces layer_s2 of models/backbones/resnet.py:16,49.  scale == shift == NULL: the bare convolution (training mode,
 * BatchNorm on batch statistics follows as its own pass). */
int egr_stem_conv7x7_f32(const float* x, egr_nmap xmap, int32_t n, int32_t h, int32_t w,
                         const float* wpack, const float* scale, const float* shift, float* y,
                         int32_t groups /* group g: x + g*gx, wpack + g*64*148, scale/shift + g*64, y + g*n*(h/2)*(w/2)*64 */,
                         int64_t gx, void* stream);

/* The same stem followed by MaxPool2d(3, 2, 1) (resnet.py:16-17: layer_s2 + layer_s4[0]) in one pass: y is (n, h/4, w/4, 64) NHWC,
 * the stride-2 tensor is never written.  Eval mode only (scale / shift required: the fused max relies on the ReLU's >= 0).
 * Bit-identical to egr_stem_conv7x7_f32 + egr_maxpool_nhwc_f32.  Two launches (a zero-fill of the pooled pixels shared
 * between tiles, then the convolution); groups as above with y + g*n*(h/4)*(w/4)*64. */
int egr_stem_conv7x7_pool_f32(const float* x, egr_nmap xmap, int32_t n, int32_t h, int32_t w,
                              const float* wpack, const float* scale, const float* shift, float* y,
                              int32_t groups, int64_t gx, void* stream);

/* The stem on the bf16 matrix cores (fp32 in / fp32 out; every operand as hi + mid + lo bf16, six products: the arithmetic of
 * EGR_W_BF16X3 launches of egr_conv2d_nhwc_f32).  w6: the filter bank split once by egr_pack_stem_w6_f32 from the [groups][64][148]
 * fp32 layout above (egr_stem_w6_bytes() bytes per group, 16-byte aligned).  pool != 0: MaxPool2d(3, 2, 1) in the same pass,
 * y = (n, h/4, w/4, 64) (eval mode only; bit-identical to pool == 0 followed by egr_maxpool_nhwc_f32); pool == 0: y = (n, h/2, w/2, 64),
 * scale == shift == NULL for the bare convolution.  h, w multiples of 64.  Replaces resnet.py:16-17,49. */
int64_t egr_stem_w6_bytes(void);
int egr_pack_stem_w6_f32(const float* w, int32_t groups, void* w6, void* stream);
int egr_stem_conv7x7_x6_f32(const float* x, egr_nmap xmap, int32_t n, int32_t h, int32_t w,
                            const void* w6, const float* scale, const float* shift, float* y,
                            int32_t pool, int32_t groups, int64_t gx, void* stream);
/* The same with the abs-max record of the pooled output (pool = 1 only; 64 uint32 slots, zero before the launch: see
 * egr_conv2d_nhwc_ex_f32) - the first residual block's convolutions take their fp16 pre-scale from it. */
int egr_stem_conv7x7_x6_ex_f32(const float* x, egr_nmap xmap, int32_t n, int32_t h, int32_t w,
                            const void* w6, const float* scale, const float* shift, float* y,
                            int32_t pool, int32_t groups, int64_t gx, uint32_t* amax_out, void* stream);
/* A Linear layer with few rows (<= 64 per launch) and a large weight matrix, as a weight stream in the fp16 scheme
 * (EgoPoseFormerPose3D.mlp_pred[0]: 2048 x 32768, models/estimator/egoposeformer_mvf_ex.py:241-253, 317-320):
 *   y[b][n] = act(sum_k x[b][k] w[n][k] + bias[n]),  n % 64 == 0, k % 256 == 0.
 * egr_pack_wstream_f32: w (n x k row-major fp32) -> image (egr_wstream_image_bytes = 4 n k bytes: two fp16 planes of w 2^k[n] in MFMA
 * fragment order) + descale[n].  egr_linear_wstream_f32: amax_in = the abs-max record of x (64 slots, as egr_conv_aux.amax_in);
 * amax_out (optional) receives max |y|; workspace of egr_linear_wstream_workspace_bytes(rows, n, k) bytes, 16-byte aligned
 * (EGR_EWORKSPACE when smaller).  Deterministic: the summation order depends on (k, n) only. */
int64_t egr_wstream_image_bytes(int32_t n, int32_t k);
int egr_pack_wstream_f32(const float* w, int32_t n, int32_t k, void* img, float* descale, void* stream);
int64_t egr_linear_wstream_workspace_bytes(int32_t rows, int32_t n, int32_t k);
int egr_linear_wstream_f32(const float* x, int64_t ldx, int32_t rows, int32_t k, const void* wimg, const float* w_descale, const float* bias,
                           int32_t n, int32_t act, const uint32_t* amax_in, float* y, int64_t ldy, uint32_t* amax_out, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* The stem in the fp16 scheme: the filter bank as two fp16 planes of w * 2^k[co] (egr_pack_stem_wh2_f32:
 * groups x egr_stem_wh2_bytes() bytes + the per-channel descale, groups x 64 floats), the input patch of a tile split on the fly after
 * a power-of-two pre-scale taken PER TILE from the patch's own largest magnitude (every k of a tile's outputs lies in that patch, so a
 * per-tile scale is a per-row scale of the GEMM: exact).  Three MFMA products per fp32 product instead of six; same operands,
 * geometry constraints, pooling and abs-max record as egr_stem_conv7x7_x6_ex_f32. */
int64_t egr_stem_wh2_bytes(void);
int egr_pack_stem_wh2_f32(const float* w, int32_t groups, void* img, float* descale, void* stream);
int egr_stem_conv7x7_h2_f32(const float* x, egr_nmap xmap, int32_t n, int32_t h, int32_t w, const void* wh2, const float* w_descale,
                            const float* scale, const float* shift, float* y, int32_t pool, int32_t groups, int64_t gx,
                            uint32_t* amax_out, void* stream);

/* MaxPool2d(k, stride, pad) on NHWC (resnet.py:17 maxpool 3/2/1; egoposeformer_mvf_ex.py:234 MaxPool2d(2)). c % 4 == 0. */
int egr_maxpool_nhwc_f32(const float* x, float* y, int32_t n, int32_t h, int32_t w, int32_t c,
                         int32_t k, int32_t stride, int32_t pad, void* stream);

/* nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True) on NHWC; c % 4 == 0.  relu != 0 applies ReLU to
 * the interpolated value: a bias-carrying 1x1 conv commutes with the interpolation (its weights sum to 1), so
 * relu(conv1x1(up(x))) is evaluated as relu(up(conv1x1(x))) at a quarter of the conv work. */
int egr_upsample2x_nhwc_f32(const float* x, int32_t ldx, float* y, int32_t ldy,
                            int32_t n, int32_t h, int32_t w, int32_t c, int32_t relu, void* stream);

/* Fold max |x| of a dense fp32 tensor of n elements into an abs-max record (64 uint32 slots, zero or holding earlier maxima: atomic
 * max on the float bits, see egr_conv2d_nhwc_ex_f32).  For tensors that enter the path from outside - e.g. the feature maps a caller
 * hands to EgoPoseFormerPose3D.forward (models/estimator/egoposeformer_mvf_ex.py:422-452) - so that their consumers can take the
 * fp16 scheme; tensors produced on the path carry the record of the launch that wrote them.  HBM-bound: one read of x. */
int egr_absmax_f32(const float* x, int64_t n, uint32_t* record, void* stream);

/* Global average pool over hw pixels of NHWC (F.adaptive_avg_pool2d(.,(1,1)), heatmap_mvf_ex.py:659). */
int egr_avgpool_nhwc_f32(const float* x, float* y, int32_t n, int32_t hw, int32_t c, void* stream);

/* utils/loss.py:122-142 get_max_preds(normalize=True): per row of `hw` = hgt*wid values: first-index argmax,
 * anchors (x/wid, y/hgt), maxvals, valid = max >= thr, raw flat index. */
int egr_argmax_rows_f32(const float* hm, int32_t rows, int32_t hgt, int32_t wid, float thr,
                        float* anchors /* rows x 2 */, float* maxvals, uint8_t* valid, int32_t* index, void* stream);

/* Soft-argmax decoding of heat maps, replaces get_max_preds_soft_pytorch (utils/loss.py:145-177; beta 1, normalize) and
 * integrate_tensor_2d (utils/util.py:80-109; beta = multiplier, mode 0 = softmax=True, mode 1 = softmax=False) - and, from the same
 * single read of the map, the hard decode of get_max_preds (utils/loss.py:122-142).  hm: `rows` dense maps (hgt, wid) fp32; z = beta*h.
 *   mode 0: p = softmax(z) over the map; mode 1: p = relu(z) / sum relu(z) (a map without positive mass gives NaN, like the 0/0 there);
 *   coords (rows, 2) = (sum p*col, sum p*row), divided by (wid, hgt) when `normalize`; maxvals = max h, index = its first flat index
 *   (the tie rule of egr_argmax_rows_f32), valid = [maxvals >= thr]; stat (rows, 2) = (max z, sum exp(z - max z) | sum relu(z)) for the
 *   backward; probs (rows, hgt, wid) or NULL: softmax(z) in mode 0, relu(z) un-normalised in mode 1 (util.py:89, 109).
 * One wave per map, fixed-order reductions, no atomics: a map's bits do not depend on the batch around it.  exp never sees a positive
 * argument, so no beta * peak overflows.  Maps with hgt*wid <= 4096, hgt*wid % 4 == 0, wid >= 4 and 16-byte aligned tensors are read
 * once into registers; every other shape below 2^24 elements takes scalar loads and reads the map twice.  EGR_EINVAL: beta not a
 * positive finite number, mode outside 0..1, hgt*wid >= 2^24. */
int egr_soft_argmax_f32(const float* hm, int32_t rows, int32_t hgt, int32_t wid, float beta, int32_t mode, int32_t normalize, float thr,
                        float* coords /* rows x 2 */, float* maxvals, int32_t* index, uint8_t* valid, float* stat /* rows x 2 */,
                        float* probs /* nullable */, void* stream);
/* Backward of the above (what autograd makes of utils/util.py:80-109 / utils/loss.py:145-177), from the forward's hm, stat, coords and
 * index:  g_hm[i] = beta p_i ((col_i - x) gx + (row_i - y) gy), p_i recomputed; (gx, gy) = g_coords, divided by (wid, hgt) when
 * `normalize`; mode 1: beta [z_i > 0] (...) / sum relu(z), and zeros for a map without positive mass (the reference's autograd gives
 * NaN there).  g_maxvals (rows) or NULL is added at `index`.  accumulate != 0 adds into g_hm.  Every element is written by one lane:
 * the same bits every run. */
int egr_soft_argmax_bwd_f32(const float* hm, const float* stat, const float* coords, const int32_t* index, const float* g_coords,
                            const float* g_maxvals /* nullable */, int32_t rows, int32_t hgt, int32_t wid, float beta, int32_t mode,
                            int32_t normalize, int32_t accumulate, float* g_hm, void* stream);
/* Coordinate L1 loss on soft-argmax joints (the role of JointsCoordinateLoss, utils/loss.py:180-200, with an L1 distance in heat-map
 * pixels): coords (rows, 2) predictions, (index, valid) the target maps' hard decode (egr_argmax_rows_f32), target = (index % wid,
 * index / wid).  loss[0] = weight / max(N_valid, 1) * sum over valid maps of |x^ - x*| + |y^ - y*| (one fp64, overwritten);
 * g_coords (rows, 2) or NULL = weight * sign(.) / max(N_valid, 1), zero where invalid.  One workgroup, fp64 sums in a fixed order. */
int egr_coord_l1_f32(const float* coords, const int32_t* index, const uint8_t* valid, int32_t rows, int32_t wid, float weight,
                     double* loss, float* g_coords /* nullable */, void* stream);

/* Fisheye triangulation: inverts utils/camera_models.py:53-104 (world2camera_pytorch, for one camera at a time - the syn rig is NOT
 * chained here, SURVEY.md F7 is a property of how the lifting head calls the projection) and intersects the rays.
 *   coords (B, V, J, 2) = (x, y) with the normalised image point (x*sx, y*sy) (heat-map pixels: sx = 1/W_hm, sy = 1/H_hm; anchors:
 *   sx = sy = 1); conf (B, V, J): a view weighs w = conf when conf >= threshold, conf > 0 and its operands are finite, else 0.
 *   cams: V records of 30 floats [npoly, cx, cy, W, H, W2C[12], nc2w, C2W[8], flip, off_x, off_y, off_z] (camera.packed_rays()).
 *   Ray: rho = |(u*W - cx, v*H - cy)|, theta from atan(C2W(rho)/rho) refined by two Newton steps on W2C(theta) = rho,
 *   d = (dx/rho cos, dy/rho cos, -sin); within 1e-4 pixels of the centre d = (0, 0, 1).
 *   Extrinsics p_cam = R p + t: ctm == NULL (syn) R = diag(f, f, 1), f = -1 where flip, t = the offset (cm); else ctm (B, V, 4, 4) in
 *   the rw convention of egr_fisheye_project_f32, p_cam = (M . [p*0.01, 1]) * 100.
 *   With P = I - d d^T:  A = sum w R^T P R,  b = -sum w R^T P t,  A p = b by LDL^T.
 * pts (B, J, 3) cm; cost (B, J) = sum w r^2 / sum w with r_v = |P_v (R_v p + t_v)| (cm^2); resid (B, V, J) = r_v, 0 for excluded
 * views; ok (B, J) = at least two views carry weight and det A > min_det_ratio * (tr A / 3)^3 - where 0, pts / cost / resid are 0.
 * One thread per (frame, joint), 64-thread workgroups, fp64 arithmetic on fp32 operands, no atomics: the same bits every run.
 * EGR_EINVAL: V outside 2..4, B or J < 1, sx / sy not positive finite, threshold NaN, min_det_ratio negative or not finite. */
int egr_triangulate_f32(const float* coords, const float* conf, const float* cams, const float* ctm /* nullable */, int32_t B, int32_t V,
                        int32_t J, float sx, float sy, float threshold, float min_det_ratio, float* pts /* B x J x 3 */,
                        float* cost /* B x J */, float* resid /* B x V x J */, uint8_t* ok /* B x J */, void* stream);
/* Backward of the above (the inverse of utils/camera_models.py:53-104 differentiated): from g_pts (B, J, 3) and g_cost (B, J), either
 * NULL for zeros, g_coords (B, V, J, 2) and g_conf (B, V, J); zero for excluded views and where ok is 0.  Through the solve
 * dp = A^-1 (db - dA p), through the cost at fixed p (the envelope theorem), through the ray with dtheta/drho = 1 / W2C'(theta).
 * The forward is recomputed from the operands (same code, same bits); a thread owns its pair's V gradients: no atomics. */
int egr_triangulate_bwd_f32(const float* coords, const float* conf, const float* cams, const float* ctm /* nullable */, int32_t B,
                            int32_t V, int32_t J, float sx, float sy, float threshold, float min_det_ratio,
                            const float* g_pts /* nullable */, const float* g_cost /* nullable */, float* g_coords, float* g_conf,
                            void* stream);

/* Volumetric fusion of multi-view heat maps into 3-D joints: the views meet before the arg-max.
 *   hm (B, V, J, H, W); conf (B, V, J): a view weighs w = conf when conf >= threshold, conf > 0 and conf is finite, else 0;
 *   centers (B, J, 3) cm, device frame; cams: V records of 30 floats (camera.packed_rays(), as for egr_triangulate_f32); ctm NULL (the
 *   syn rig, un-chained) or (B, V, 4, 4) in the rw convention - p_cam = R p + t exactly as egr_triangulate_f32 defines R and t;
 *   center_ok (B, J) or NULL: a 0 marks a centre that is not to be used (the `ok` of the triangulation that made it).
 *   Voxel i = (iz*G + iy)*G + ix of the cube of side `cube` cm sits at p_i = c + o_i, o_i = ((ix+.5)/G - .5, (iy+.5)/G - .5,
 *   (iz+.5)/G - .5) * cube.  Projection q = R p + t, n = |(qx, qy)|, theta = atan2(-qz, n), rho = W2C(theta), pixel
 *   ((qx/n) rho + cx, (qy/n) rho + cy) - direction (0, 0) where n == 0 - heat-map coordinate (x, y) = (px * W / W_img, py * H / H_img),
 *   unclamped; a voxel with n == 0 and qz <= 0 takes no sample from that view.  Sample s: bilinear between the integer indices around
 *   (x, y), a corner outside the map counts 0, a non-finite coordinate gives 0.  S_i = sum_v w_v s_vi / sum_v w_v.
 * peak (B, J) = max_i S_i; index (B, J) = the first voxel attaining it; with P = softmax_i(beta * S_i): pose (B, J, 3) = c + sum_i P_i o_i
 * and spread (B, J) = sqrt(sum_i P_i |o_i - (pose - c)|^2), cm.  ok (B, J) = at least two views carry weight, the centre is finite and
 * center_ok allows it - where 0: pose = peak = spread = 0 and index = -1.
 * One 512-thread workgroup per (frame, joint), the pair's maps staged in LDS once, an online softmax per thread, the records merged
 * in a fixed order; fp64 arithmetic on fp32 operands, no atomics: the same bits every run, alone or in a batch.
 * EGR_EINVAL: V outside 2..4, G outside 2..32, V*H*W > 16384, B / J / H / W < 1, cube or beta not positive finite, threshold NaN. */
int egr_volume_fuse_f32(const float* hm, const float* conf, const float* centers, const float* cams, const float* ctm /* nullable */,
                        const uint8_t* center_ok /* nullable */, int32_t B, int32_t V, int32_t J, int32_t H, int32_t W, int32_t G,
                        float cube, float beta, float threshold, float* pose /* B x J x 3 */, float* peak /* B x J */,
                        int32_t* index /* B x J */, float* spread /* B x J */, uint8_t* ok /* B x J */, void* stream);
/* Backward of the above with respect to hm (conf and centers are constants: the cube is placed, not learned): from g_pose (B, J, 3) and
 * g_peak (B, J), either NULL for zeros, g_hm (B, V, J, H, W).  gS_i = beta P_i ((o_i - (pose - c)) . g_pose) + [i == index] g_peak,
 * and each of the four corners of each view's sample receives gS_i * w_v / sum w * (its bilinear weight); zero for excluded views and
 * where ok is 0.  One 1024-thread workgroup per (frame, joint); the scores are recomputed from the maps in LDS (the forward's code),
 * the gradients of the pair's maps are summed in a second LDS image (fp32 LDS adds, whose order is not fixed: the last bits may differ
 * between runs) and every element of g_hm is written once with a plain store - no global atomics, g_hm need not be zeroed. */
int egr_volume_fuse_bwd_f32(const float* hm, const float* conf, const float* centers, const float* cams, const float* ctm /* nullable */,
                            const uint8_t* center_ok /* nullable */, int32_t B, int32_t V, int32_t J, int32_t H, int32_t W, int32_t G,
                            float cube, float beta, float threshold, const float* g_pose /* nullable */,
                            const float* g_peak /* nullable */, float* g_hm, void* stream);

/* Multi-peak decoding of heat maps: the K best local maxima of every map, refined to sub-pixel.
 *   hm: `rows` dense maps (hgt, wid) fp32, 1 <= hgt*wid <= 4096.  A NaN compares as -inf; +-inf compare as they are; pixels outside the
 *   map count as -inf.  Pixel i (flat index) is a peak when h_i is finite, h_i > min_score, h_i > h_n for every neighbour n < i of its
 *   (2*nms_radius+1)^2 window and h_i >= h_n for every neighbour n > i: a plateau keeps its first pixel, a constant map the peak 0.
 *   The K best peaks by value, ties to the smaller flat index (the rule of egr_soft_argmax_f32), are kept in that order.  A kept peak
 *   (cm, rm) of value m is refined over its (2*refine_radius+1)^2 window clipped to the map: e_p = exp(beta (h_p - m)) for finite h_p,
 *   else 0;  x = cm + sum e_p (col_p - cm) / sum e_p, y likewise - heat-map pixels, the convention of egr_soft_argmax_f32.
 * coords (rows, K, 2); score (rows, K) = the peak's value, copied; index (rows, K) = its flat index; count (rows) = peaks kept.  A
 * slot past count holds coords 0, score 0, index -1.
 * One wave - one 64-thread workgroup - per map; the map is read once and staged in LDS; fixed-order reductions, fp64 refinement, no
 * atomics: the same bits every run, alone or in a batch.
 * EGR_EINVAL: hgt*wid outside 1..4096, K outside 1..4, nms_radius outside 1..3, refine_radius outside 0..3, beta not positive finite,
 * min_score not finite. */
int egr_peaks_f32(const float* hm, int32_t rows, int32_t hgt, int32_t wid, int32_t K, int32_t nms_radius, int32_t refine_radius, float beta,
                  float min_score, float* coords /* rows x K x 2 */, float* score /* rows x K */, int32_t* index /* rows x K */,
                  int32_t* count /* rows */, void* stream);
/* Consensus over the views' candidate peaks: per (frame, joint) the candidates the views agree on.
 *   cand (B, V, J, K, 2), cscore (B, V, J, K), cindex (B, V, J, K): the outputs of egr_peaks_f32; a candidate exists when its index is
 *   >= 0, its score finite and > 0 and its coordinates finite.  cams, ctm, sx, sy, min_det_ratio as for egr_triangulate_f32.
 *   Hypothesis h = (pair(a, b)*K + ka)*K + kb over the view pairs a < b in lexicographic order, both candidates existing: its point p
 *   is egr_triangulate_f32's intersection of the two rays weighted by the two scores (the same ok).  p is projected into every view
 *   (R p + t, the unclamped projection of egr_volume_fuse_f32) and taken to coords units by 1 / (sx W_img), 1 / (sy H_img).  View v
 *   supports h with its largest  cscore_vk * max(0, 1 - e^2 / max_reproj^2),  e the distance between the projection and candidate k,
 *   ties to the smaller k; its choice is that k, or -1 when the support is 0 or the projection does not exist.  score_h = the sum of
 *   the views' support, inliers_h = the views with a choice.  The winner: the largest score among the hypotheses with inliers >=
 *   min_views, ties to the smaller h.
 * choice (B, V, J); sel_coords (B, V, J, 2) and sel_conf (B, V, J) = the chosen candidate's coords and score, copied, 0 where the choice
 * is -1: the operands of egr_triangulate_f32.  score (B, J), inliers (B, J), hyp (B, J) = the winner's; hyp -1, score 0, inliers 0 and
 * every choice -1 where no hypothesis qualifies.
 * One wave per (frame, joint), lanes = hypotheses; fp64 arithmetic on fp32 operands, a fixed-order arg-max, no atomics: the same bits
 * every run, alone or in a batch.
 * EGR_EINVAL: V outside 2..4, K outside 1..4, B or J < 1, sx / sy / max_reproj not positive finite, min_views outside 2..V,
 * min_det_ratio negative or not finite. */
int egr_consensus_f32(const float* cand, const float* cscore, const int32_t* cindex, const float* cams, const float* ctm /* nullable */,
                      int32_t B, int32_t V, int32_t J, int32_t K, float sx, float sy, float max_reproj, int32_t min_views,
                      float min_det_ratio, int32_t* choice /* B x V x J */, float* sel_coords /* B x V x J x 2 */,
                      float* sel_conf /* B x V x J */, float* score /* B x J */, int32_t* inliers /* B x J */, int32_t* hyp /* B x J */,
                      void* stream);

/* Bone-length-constrained skeleton fit over the fisheye rays.  Per frame, over the active joints p_j (cm, device frame)
 * of a tree of J <= 16 joints, minimise
 *   E(p) = sum_j sum_v w_vj dist^2(p_j, ray_vj) + lambda sum_{j > 0, bone j used} (|p_j - p_parent(j)| - L_j)^2 + rho sum_j |p_j - init_j|^2.
 *   coords, conf, cams, ctm, sx, sy, threshold, min_det_ratio as for egr_triangulate_f32: the same rays, the same views used or
 *   excluded, w = conf.  parents: J int32 in HOST memory, parents[0] == 0 and 0 <= parents[j] < j (checked here; it travels to the
 *   kernel by value).  bone_length (J), or (B, J) with bone_length_per_frame != 0, cm: entry 0 is ignored, an entry <= 0 or not finite
 *   leaves that bone unconstrained.  init (B, J, 3) cm and init_ok (B, J): an init with a non-finite component counts as not ok.
 *   Active joints, decided once per frame in index order: with rho > 0 a joint is active iff its init is ok; with rho == 0 iff its
 *   init is ok and either its own rays fix it (egr_triangulate_f32's ok: two used views or more and the normal equations factor) or it
 *   has at least one used view and a constrained bone to an active parent.  A joint is never anchored from a child: a joint whose
 *   only support is a bone to a child below it is not active at rho == 0.  A bone is used iff both ends are active and its length is
 *   constrained; a bone shorter than 1e-9 cm contributes its constant residual and no gradient.
 *   Solver: Levenberg-Marquardt on the Gauss-Newton model (the data and prior terms are exact quadratics, a used bone contributes
 *   lambda u u^T blocks, u = d / |d|): every iteration solves (H + mu diag H) delta = -g at the current p - eliminated along the tree
 *   from the deepest joints to the roots in 3 x 3 LDL^T steps, a parent folding its children in index order, then back-substituted -
 *   and keeps p + delta iff every block factored and E(p + delta) <= E(p) - the change evaluated as a difference (exactly for the
 *   quadratic terms, through len' - len for a bone), so that steps below the rounding of E are still decided.  mu starts at 1e-3; a kept step multiplies it by 0.1 (not
 *   below 1e-12), a refused one by 10 (not above 1e12).  `iterations` (1..256) such iterations run, always.  One block that does not
 *   factor refuses the step for the whole frame.  Convergence is linear: where bones end under tension or compression and the rays
 *   are soft along the viewing direction, fp32 stationarity can take more than the 256 iterations (`grad` says how far it got).
 * pose (B, J, 3): 0 where not valid; ray_cost (B, J): sum_v w dist^2 / sum_v w at the fitted point (egr_triangulate_f32's cost), 0
 * without a used view; bone (B, J): the fitted length, 0 for the root and for a bone that is not used; valid (B, J): 1 when active;
 * energy0 (B), energy (B): E at the init and at the result, each the three sums evaluated there (no kept step raises E, so energy
 * <= energy0 up to the rounding of the two sums: an fp32 ulp of energy0 at most, where no step lowered it); grad (B): the largest
 * |dE/dp| component over the active joints at the result; steps (B): the kept steps.  A frame without an active joint gives zeros.
 * One wave per frame: lane v*16 + j builds the ray of view v of joint j once, lane j owns joint j's block, parents and children
 * exchange by cross-lane reads; fp64 arithmetic on fp32 operands, no atomics, no LDS: the same bits every run, alone or in a batch.
 * EGR_EINVAL: the shapes egr_triangulate_f32 refuses, J > 16, a bad parent table, lambda or rho negative or not finite, iterations
 * outside 1..256. */
int egr_skeleton_fit_f32(const float* coords, const float* conf, const float* cams, const float* ctm /* nullable */,
                         const int32_t* parents /* J, host */, const float* bone_length, int32_t bone_length_per_frame, const float* init,
                         const uint8_t* init_ok, int32_t B, int32_t V, int32_t J, float sx, float sy, float threshold, float min_det_ratio,
                         float lambda, float rho, int32_t iterations, float* pose /* B x J x 3 */, float* ray_cost /* B x J */,
                         float* bone /* B x J */, uint8_t* valid /* B x J */, float* energy0 /* B */, float* energy /* B */,
                         float* grad /* B */, int32_t* steps /* B */, void* stream);
/* Bone statistics of a clip: pose (B, J, 3), valid (B, J), parents as above (host) -> length (J), spread (J) - mean and (population)
 * standard deviation of |p_j - p_parent(j)| over the frames in which both ends are valid - and count (J), those frames.  Entry 0 and a
 * bone with count 0 give 0.  One thread per bone, fp64 sums in frame order (the mean, then the deviations): bit-reproducible. */
int egr_bone_lengths_f32(const float* pose, const uint8_t* valid, const int32_t* parents /* J, host */, int32_t B, int32_t J, float* length,
                         float* spread, int32_t* count, void* stream);
/* Skeleton._skeleton_resize (pose_estimation/utils/skeleton.py:163-174) in cm (the reference works in mm and divides by 1000; nothing
 * is divided here): the tree is walked in index order, out_j = out_parent(j) + (p_j - p_parent(j)) * L_j / |p_j - p_parent(j)|, the
 * direction taken from the input pose.  A joint with valid 0 keeps its place, and so does a joint whose parent is not valid - it
 * starts a chain of its own.  A bone whose length is <= 0 or not finite, or shorter than 1e-9 cm in the input, keeps its vector.
 * bone_length (J), or (B, J) with bone_length_per_frame != 0.  One thread per frame; out must not be pose. */
int egr_skeleton_resize_f32(const float* pose, const uint8_t* valid, const int32_t* parents /* J, host */, const float* bone_length,
                            int32_t bone_length_per_frame, int32_t B, int32_t J, float* out /* B x J x 3 */, void* stream);

/* Temporal trajectory smoothing of 3-D joints over a clip.  A track is one joint of one clip: observations z_t =
 * pose[n, t, j, :] (cm), t = 0..T-1, with base weights  w_t = weight_t [obs_t != 0] [z_t and weight_t finite, weight_t > 0]  (weight
 * NULL: 1; obs NULL: every frame; egr_triangulate_f32's ok plugs in as obs).  A frame with w_t = 0 is never read into arithmetic: what
 * is planted there reaches no output.  The smoothed track minimises
 *   E(x) = sum_t w_t rho(|x_t - z_t|) + vel_weight sum_{t=0}^{T-2} |x_{t+1} - x_t|^2 + accel_weight sum_{t=1}^{T-2} |x_{t+1} - 2 x_t + x_{t-1}|^2,
 * rho(r) = r^2 with huber == 0;  r^2 for r <= huber and 2 huber r - huber^2 beyond with huber > 0.
 *   Plain form (huber == 0, reweights == 0): x solves A x = W z, A = W + vel_weight D1^T D1 + accel_weight D2^T D2 - symmetric,
 *   positive definite, pentadiagonal, shared by the three coordinates.
 *   Robust form (huber > 0, reweights = K in 1..16): s(0) = 1; x(k) solves the plain problem with the weights w_t s_t(k);
 *   s_t(k+1) = min(1, huber / |x_t(k) - z_t|); the result is x(K) - K + 1 solves, always, no convergence test.  A majorise-minimise
 *   step: E does not increase from one k to the next.
 *   A track is solvable (A positive definite), decided from the base weights: with vel_weight > 0, one observed frame or more; with
 *   vel_weight == 0 and T >= 3, two or more; with vel_weight == 0 and T <= 2, every frame.  A track that is not solvable gives pose 0,
 *   valid 0, residual 0, weight_out 0 and energy 0.
 * pose_out (N, T, J, 3): written for every frame of a solvable track; valid (N, T, J): 1 iff the track is solvable and the nearest
 * observed frame is at most max_gap frames away; residual (N, T, J): |x_t - z_t| at observed frames, 0 elsewhere; weight_out
 * (N, T, J): w_t s_t(K), the weights of the last solve; energy (N, J): E at the result, rho as configured, with the base weights.
 * workspace: 5 * T * N * J doubles, contents unspecified before and after.  The parameters are taken as fp32.
 * One lane per track, a banded LDL^T along t in fp64 on the fp32 operands, every solve and the energy pass in the one launch; no
 * atomics, a fixed order: the same bits every run, alone or in a batch.  Latency-bound: a dependent fp64 chain of length T per sweep.
 * EGR_EINVAL: N or J < 1, T outside 1..4096, N*T*J >= 2^31, a weight negative or not finite or both zero, huber negative or not
 * finite, reweights outside 0..16, reweights > 0 with huber == 0 or huber > 0 with reweights == 0, max_gap < 0. */
int egr_trajectory_smooth_f32(const float* pose, const float* weight /* nullable */, const uint8_t* obs /* nullable */, int32_t N, int32_t T,
                              int32_t J, float vel_weight, float accel_weight, float huber, int32_t reweights, int32_t max_gap,
                              double* workspace /* 5 x T x N x J */, float* pose_out /* N x T x J x 3 */, uint8_t* valid /* N x T x J */,
                              float* residual /* N x T x J */, float* weight_out /* N x T x J */, float* energy /* N x J */, void* stream);
/* Backward of the plain form: with u = A^-1 g_pose_out (the same factorisation, recomputed from the operands, on three more
 * right-hand sides)  g_pose[t] = w_t u_t  and  g_weight[t] = [observed_t] u_t . (z_t - x_t)  (g_weight NULL to skip); zeros for a track
 * that is not solvable.  workspace: 8 * T * N * J doubles.  EGR_EINVAL as above. */
int egr_trajectory_smooth_bwd_f32(const float* pose, const float* weight /* nullable */, const uint8_t* obs /* nullable */,
                                  const float* g_pose_out /* N x T x J x 3 */, int32_t N, int32_t T, int32_t J, float vel_weight,
                                  float accel_weight, double* workspace /* 8 x T x N x J */, float* g_pose /* N x T x J x 3 */,
                                  float* g_weight /* N x T x J, nullable */, void* stream);

/* Causal fixed-lag filter of streamed 3-D joints: egr_trajectory_smooth_f32's plain form, one frame at a time.  A stream
 * is one joint's observations z_0, z_1, ... with the base weights w_t above.  The used weights are u_t = w_t, or with gate = delta > 0
 *   u_t = w_t min(1, delta / |z_t - p_t|),  p_t = frame t of the plain solution over the frames 0..t with the weights u_0..u_{t-1}, 0,
 * wherever that system is solvable (else u_t = w_t); a weight is fixed once assigned.  x^(t) is the plain solution over the frames 0..t
 * with the weights u (zeros where that prefix is not solvable, by the rule above with T = t + 1).  The arrival of frame t describes stream
 * frame t - lag: pose x^(t)_{t-lag}; valid iff the prefix is solvable and the nearest observed frame within 0..t is at most max_gap
 * away; residual |x - z| there if observed, else 0; weight u there; frame = t - lag.  While t < lag the row is zeros with frame -1.
 * The C frames pose[n, c] of a call arrive one after another; outputs and state do not depend on how a stream is cut into calls.
 * reset[n] != 0 empties stream n before the call's first frame: slots 0..22 start from zero; the ring rows of the earlier stream stay
 * in the tensor and are never read (a substitution reaches only rows committed since the reset), so after a reset the outputs are
 * those of a new state, the tensor's ring slots need not be.
 *   state: egr_trajectory_filter_state_slots(lag) x N x J doubles, laid out (slot, track), track = n * J + j; all zeros is the empty
 *   stream; updated in place.  Slots: 0..10 the elimination's chain d1, d2, e1, f1, f2, y1[3], y2[3] after the last final row (t - 2);
 *   11..15 frame t - 1 and 16..20 frame t: u, z[3], frames since the last observed one; 21 frames seen; 22 observed frames seen,
 *   saturating at 2; 23 + 10 r .. 32 + 10 r the final row s with s mod lag = r: e, f, q[3], z[3], u, frames since the last observed
 *   one.  Everything the arithmetic needs is there: a call can be captured into a graph once and replayed every frame.  Streams have
 *   no length limit (slot 21 is exact up to 2^53 frames).
 * One lane per track, fp64 on the fp32 operands, no atomics, a fixed order: a track's bits depend on its own operands only.
 * EGR_EINVAL: N, C or J < 1, C > 4096, lag outside 0..64, N*C*J or N*J*slots >= 2^31, a penalty weight negative or not finite or both
 * zero, gate negative or not finite, max_gap < 0. */
int64_t egr_trajectory_filter_state_slots(int32_t lag); /* 23 + 10 lag; EGR_EINVAL for lag outside 0..64 */
int egr_trajectory_filter_f32(const float* pose /* N x C x J x 3 */, const float* weight /* N x C x J, nullable */,
                              const uint8_t* obs /* N x C x J, nullable */, const uint8_t* reset /* N, nullable */,
                              double* state /* slots x N x J */, int32_t N, int32_t C, int32_t J, int32_t lag, float vel_weight,
                              float accel_weight, float gate, int32_t max_gap, float* pose_out /* N x C x J x 3 */,
                              uint8_t* valid /* N x C x J */, float* residual /* N x C x J */, float* weight_out /* N x C x J */,
                              int64_t* frame /* N x C */, void* stream);
/* The part no arrival has described yet: with T frames seen, rows 0..lag-1 are the frames T - lag .. T - 1 of x^(T-1), with the five
 * outputs above; a row before the stream's start is zeros with frame -1.  The last row is the causal estimate of the present.  The
 * state is read, not written.  lag == 0: no rows, nothing is launched. */
int egr_trajectory_filter_tail_f32(const double* state /* slots x N x J */, int32_t N, int32_t J, int32_t lag, float vel_weight,
                                   float accel_weight, int32_t max_gap, float* pose_out /* N x lag x J x 3 */,
                                   uint8_t* valid /* N x lag x J */, float* residual /* N x lag x J */, float* weight_out /* N x lag x J */,
                                   int64_t* frame /* N x lag */, void* stream);

/* Rig self-calibration: the cameras' rotations refined from the decoded 2-D joints of a clip.  Over the pairs
 * (frame b, joint j), with the rays, weights and extrinsics of egr_triangulate_f32 (the same views used or excluded, w = conf),
 *   E(dR_0..dR_{V-1}) = sum_pairs min_p sum_v w_v |P(dR_v^T d_v) (R_v p + t_v)|^2 + prior_weight sum_v |dR_v - I|_F^2,  P(d) = I - d d^T,
 * dR_v a rotation of camera v about its own centre: p_cam' = dR_v (R_v p + t_v), M'_v = [dR_v 0; 0 1] M_v.  Translations are not
 * refined: a ray-distance cost with free translations collapses the rig.  ctm: NULL (the syn rig), or (B, V, 4, 4) with
 * ctm_per_frame != 0, or (1, V, 4, 4) for the clip with ctm_per_frame == 0.  fixed_mask: bit v holds camera v at dR = I (every bit
 * set is legal: the result is the identity and cost == cost0).
 *   A pair counts - decided once, at dR = I - when two views or more carry weight and its 3 x 3 normal equations pass
 *   egr_triangulate_f32's test with min_det_ratio.  Later iterates solve the same pairs with the positivity test alone; a candidate at
 *   which a counted pair fails is refused like one that raises E.
 *   Solver: Levenberg-Marquardt on the Gauss-Newton model, the point of every pair eliminated by its 3 x 3 Schur complement, the local
 *   update dR_v <- exp([delta_v]x) dR_v, the prior's gradient and exact Hessian at delta = 0 added.  mu starts at 1e-4; every
 *   iteration solves (H + mu diag H) delta = -g over the free cameras at the accepted rotations (LDL^T), evaluates the candidate, and
 *   keeps it iff every counted pair factors and E falls strictly - mu then times 0.1 (not below 1e-12); a refused one multiplies mu by
 *   10 (not above 1e12) and the next iteration solves again from the stored system.  `iterations` (1..256) candidates are tried,
 *   always: 1 + 2 (iterations + 1) launches on `stream`, all solver state in `workspace`, no host synchronisation.
 * rotation (V, 3): the rotation vectors of dR, rad; matrix (V, 3, 3): dR; ctm_out (B, V, 4, 4): [matrix 0; 0 1] M in the decoders'
 * convention (translations in m) - for the syn rig M is diag(f, f, 1) with f = -1 for a flipped camera and the record's offset * 0.01
 * as fp32 - the product of the fp32 matrices formed in fp64 and rounded once; cost0, cost (1 each): sum w dist^2 / sum w over the counted pairs before and after, cm^2
 * (egr_triangulate_f32's cost, pooled); pairs (1): the counted pairs; steps (1): the kept candidates; grad (1): the largest |dE/d delta|
 * component over the free cameras at the result; valid (1): 0 when no pair counts, the start is not finite or its undamped system does
 * not factor (a pivot at or below 1e-10 of its diagonal entry) - then every rotation is the identity, ctm_out is M and the scalars are 0.
 * workspace: egr_rig_refine_workspace_bytes(B, V, J) bytes (0 for shapes the entry refuses), contents unspecified before and after.
 * One thread per pair and iteration, the 94 sums of a pair reduced in a fixed order - an xor butterfly of wave shuffles, the waves of a
 * workgroup in LDS in wave order, one record a workgroup, the records in block order by the one workgroup of the step kernel: no
 * atomics, the same bits every run whatever the grid's scheduling.  fp64 arithmetic on fp32 operands.
 * EGR_EINVAL: the shapes egr_triangulate_f32 refuses, B * J >= 2^28, fixed_mask outside 0..2^V - 1, prior_weight negative or not
 * finite, iterations outside 1..256; EGR_EWORKSPACE: workspace_bytes too small. */
int64_t egr_rig_refine_workspace_bytes(int32_t B, int32_t V, int32_t J);
int egr_rig_refine_f32(const float* coords, const float* conf, const float* cams, const float* ctm /* nullable */, int32_t ctm_per_frame,
                       int32_t B, int32_t V, int32_t J, float sx, float sy, float threshold, float min_det_ratio, int32_t fixed_mask,
                       float prior_weight, int32_t iterations, double* workspace, int64_t workspace_bytes, float* rotation /* V x 3 */,
                       float* matrix /* V x 3 x 3 */, float* ctm_out /* B x V x 4 x 4 */, float* cost0, float* cost, int32_t* pairs,
                       int32_t* steps, float* grad, uint8_t* valid, void* stream);

/* Ray-space clip smoothing: the 3-D tracks of a clip fitted to the views' rays directly.  A track is one joint j of one
 * clip n, T frames; with the rays, weights and extrinsics of egr_triangulate_f32 at frame b = n T + t (w_tv = conf where the view is
 * used - conf >= threshold, conf > 0, conf and coords finite - else 0, and what stands there is never read) it minimises over x_0..x_{T-1} (cm)
 *   E(x) = sum_t sum_v w_tv rho(|P_tv (R_tv x_t + t_tv)|) + vel_weight sum_{t=0}^{T-2} |x_{t+1} - x_t|^2
 *                                                         + accel_weight sum_{t=1}^{T-2} |x_{t+1} - 2 x_t + x_{t-1}|^2,   P = I - d d^T,
 * rho as in egr_trajectory_smooth_f32 (the square, or Huber's function of the ray distance at huber > 0).  coords (N, T, V, J, 2),
 * conf (N, T, V, J), cams (V, 30) ray records, ctm NULL (the syn rig) or (N, T, V, 4, 4).  A frame without a used ray is a gap that
 * its neighbours fill; a frame with one used ray contributes that ray: two of the point's three degrees of freedom.
 *   Plain form: x solves the 3T x 3T system  (blockdiag(G_t) + (vel_weight D1^T D1 + accel_weight D2^T D2) (x) I_3) x = (g_t),
 *   G_t = sum_v w_tv R^T P R and g_t = -sum_v w_tv R^T P t the normal equations of frame t's rays - block pentadiagonal.
 *   Robust form (huber > 0, reweights = K in 1..16): x(0) the plain solve; x(k+1) solves the plain problem with the ray weights
 *   w_tv min(1, huber / dist_tv(x(k))); K + 1 solves, always.  E does not increase from one k to the next.
 *   A track is solvable when (a) with vel_weight > 0 it has 2 used rays or more; with vel_weight == 0 and T >= 3, 3 used rays or more
 *   on 2 frames or more; with vel_weight == 0 and T <= 2, 2 used rays or more in every frame; and (b) every scalar pivot of the
 *   elimination below, in the plain solve, exceeds min_pivot_ratio x the largest diagonal entry of the track's matrix (a NaN fails).
 *   A track that is not solvable gives 0 in every output.
 *   Elimination: block LDL^T along t without pivoting, D_t = G_t + a_t I - E_{t-1} D_{t-1} E_{t-1}^T - F_{t-2} D_{t-2} F_{t-2}^T with
 *   (a_t, b_t, c_t) row t of the penalty, E_t = (b_t I - c_{t-1} E_{t-1}^T) D_t^-1, F_t = c_t D_t^-1; every D_t by the 3 x 3 LDL^T of
 *   the triangulation (no pivoting, coordinate order x, y, z): its three d are the scalar pivots of rule (b), 3T a track.
 * pose (N, T, J, 3): written for every frame of a solvable track; valid (N, T, J): 1 iff the track is solvable and a frame with a used
 * ray is at most max_gap frames away; residual (N, T, V, J): the ray distance at the result for used rays, 0 elsewhere; weight
 * (N, T, V, J): the ray weights of the last solve; rays (N, T, J): the number of used rays; energy (N, J): E at the result with the
 * base weights.  workspace: egr_ray_track_workspace_bytes(N, T, V, J) bytes = (4 V + 18) T N J doubles (0 for shapes the entry
 * refuses), contents unspecified before and after.  The parameters are taken as fp32 except min_pivot_ratio.
 * Two launches on `stream`, no host synchronisation: the ray pass (a thread per (frame, joint): the views' unit rays and weights in
 * fp64, planes of T x N J), then the solve - one lane per track, the tracks of a clip in adjacent lanes, every sweep of the K + 1
 * solves and the energy pass inside it.  No atomics, a fixed order: the same bits every run, alone or in a batch.  Latency-bound.
 * EGR_EINVAL: N or J < 1, V outside 2..4, T outside 1..4096, N*T*V*J*2 >= 2^31, sx or sy not positive and finite, threshold NaN, the
 * penalties, huber, reweights and max_gap as egr_trajectory_smooth_f32 refuses them, min_pivot_ratio negative, NaN or >= 1;
 * EGR_EWORKSPACE: workspace_bytes too small. */
int64_t egr_ray_track_workspace_bytes(int32_t N, int32_t T, int32_t V, int32_t J);
int egr_ray_track_f32(const float* coords, const float* conf, const float* cams, const float* ctm /* nullable */, int32_t N, int32_t T,
                      int32_t V, int32_t J, float sx, float sy, float threshold, float vel_weight, float accel_weight, float huber,
                      int32_t reweights, int32_t max_gap, double min_pivot_ratio, double* workspace, int64_t workspace_bytes,
                      float* pose /* N x T x J x 3 */, uint8_t* valid /* N x T x J */, float* residual /* N x T x V x J */,
                      float* weight /* N x T x V x J */, uint8_t* rays /* N x T x J */, float* energy /* N x J */, void* stream);

/* Information-weighted clip smoothing, two entries.
 * egr_joint_info_f32: the information matrix of a 3-D point under the views that see it.  points (B, J, 3) cm in the device frame,
 * conf (B, V, J), cams (V, 30) ray records, ctm NULL (the syn rig, each camera on its own) or (B, V, 4, 4) - the extrinsics of
 * egr_triangulate_f32.  With c_v(p) the coordinates of the point in view v in the units of `coords` everywhere in the decoders (image
 * pixels / (sx W_img, sy H_img): heat-map pixels for sx = 1 / W) and J_v = d c_v / d p (2 x 3)
 *   W = sum_v conf_v J_v^T J_v   over the views that enter:
 * conf >= threshold, conf > 0, conf finite (egr_triangulate_f32's rule), and the point gives a pixel off the optical axis - the
 * camera-frame point q = R p + t is finite with n = |q_xy| > 0.  A view that does not enter weighs nothing and nothing of it is read
 * into an output; a point that is not finite gives zeros, views 0, valid 0.  No coordinates are taken: W depends on where the point
 * is, not on where it was observed.  J_v is analytic: theta = atan2(-q_z, n), rho(theta) and rho'(theta) of the W2C polynomial (Horner).
 * info (B, J, 6): W in the order (00, 01, 02, 11, 12, 22); views (B, J): the views that entered; valid (B, J): W passes
 * egr_triangulate_f32's LDL^T test with min_det_ratio; sigma (B, J) = sqrt(trace(W^-1)) where valid - cm of positional standard
 * deviation per unit of coordinate noise - else 0.  One thread per (frame, joint), fp64 arithmetic on fp32 operands, a fixed order over
 * the views, no atomics.  EGR_EINVAL: the shapes, scales and min_det_ratio egr_triangulate_f32 refuses, threshold NaN.
 *
 * egr_info_track_f32: the clip smoother with one such matrix a frame.  A track is one joint j of one clip n, T frames of observations
 * z_t = pose[n, t, j] (cm) with W_t = info[n, t, j]; it minimises over x_0..x_{T-1}
 *   E(x) = sum_t rho(r_t) + vel_weight sum_{t=0}^{T-2} |x_{t+1} - x_t|^2 + accel_weight sum_{t=1}^{T-2} |x_{t+1} - 2 x_t + x_{t-1}|^2,
 *   r_t = sqrt((x_t - z_t)^T W_t (x_t - z_t))   - the displacement in coordinate units (pixels) -
 * over the frames that are used: obs != 0 (NULL: every frame), pose and the six entries finite, every diagonal entry >= 0 and the
 * trace > 0.  Any other frame is a gap that its neighbours fill, and what stands there is never read.  A positive semi-definite W of
 * rank 2 (one view) is a legitimate frame.  rho is the square, or Huber's function at huber > 0 (in pixels: r_t has the noise's units).
 *   Plain form: x solves (blockdiag(W_t) + (vel_weight D1^T D1 + accel_weight D2^T D2) (x) I_3) x = (W_t z_t) - egr_ray_track_f32's
 *   system with G_t = W_t, g_t = W_t z_t, and its elimination (block LDL^T without pivoting, the same code).
 *   Robust form (huber > 0, reweights = K in 1..16): x(0) the plain solve; x(k+1) solves the plain problem with s_t W_t,
 *   s_t = min(1, huber / r_t(x(k))); K + 1 solves, always.  E does not increase from one k to the next.
 *   A track is solvable when (a) it has enough used frames for its penalties - 1 with vel_weight > 0; with vel_weight == 0, 2 where
 *   T >= 3 and every frame where T <= 2 - and (b) every scalar pivot of the plain solve's elimination exceeds min_pivot_ratio x the
 *   largest diagonal entry of the track's matrix (a NaN fails).  A track that is not solvable gives 0 in every output.
 * pose_out (N, T, J, 3): written for every frame of a solvable track; valid (N, T, J): 1 iff the track is solvable and a used frame is
 * at most max_gap frames away; residual (N, T, J): r_t at the result for used frames, 0 elsewhere; weight (N, T, J): s_t of the last
 * solve (1 in the plain form), 0 for a gap; energy (N, J): E at the result.  workspace: egr_info_track_workspace_bytes(N, T, J) bytes
 * = 18 T N J doubles (0 for shapes the entry refuses), contents unspecified before and after.  The parameters are taken as fp32 except
 * min_pivot_ratio.  One launch: one lane per track, the tracks of a clip in adjacent lanes, every sweep of the K + 1 solves and the
 * energy pass inside it.  No atomics, a fixed order: the same bits every run, alone or in a batch.  Latency-bound.
 * EGR_EINVAL: N or J < 1, T outside 1..4096, N*T*J*6 >= 2^31, the penalties, huber, reweights and max_gap as
 * egr_trajectory_smooth_f32 refuses them, min_pivot_ratio negative, NaN or >= 1; EGR_EWORKSPACE: workspace_bytes too small. */
int egr_joint_info_f32(const float* points, const float* conf, const float* cams, const float* ctm /* nullable */, int32_t B, int32_t V,
                       int32_t J, float sx, float sy, float threshold, float min_det_ratio, float* info /* B x J x 6 */,
                       uint8_t* views /* B x J */, float* sigma /* B x J */, uint8_t* valid /* B x J */, void* stream);
int64_t egr_info_track_workspace_bytes(int32_t N, int32_t T, int32_t J);
int egr_info_track_f32(const float* pose, const float* info, const uint8_t* obs /* nullable */, int32_t N, int32_t T, int32_t J,
                       float vel_weight, float accel_weight, float huber, int32_t reweights, int32_t max_gap, double min_pivot_ratio,
                       double* workspace, int64_t workspace_bytes, float* pose_out /* N x T x J x 3 */, uint8_t* valid /* N x T x J */,
                       float* residual /* N x T x J */, float* weight /* N x T x J */, float* energy /* N x J */, void* stream);

/* y = LayerNorm(x (+ res)) * gamma + beta over the last dim c (c <= 1024, c % 64 == 0), eps 1e-5. */
int egr_layernorm_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                      int32_t rows, int32_t c, float eps, int32_t rows_per_group /* gamma/beta + (row/rows_per_group)*c; 0 = one group */,
                      void* stream);

/* Joint-to-joint attention core of SpatialMHA / EgoformerSpatialMHA (heatmap_mvf_ex.py:799-817,
 * egoposeformer_mvf_ex.py:481-498): qkv (b, j, 3*c) -> out (b, j, c); softmax(q k^T * scale) v per head; j <= 16. */
int egr_joint_mha_f32(const float* qkv, float* out, int32_t b, int32_t j, int32_t heads, int32_t d, float scale, void* stream);

/*
 * Deformable-attention sampling in sample-then-project form (replaces the mmcv CUDA op
 * MultiScaleDeformableAttnFunction, models/utils/deform_attn.py:155-162, together with the
 * softmax / location arithmetic of :122-137).  For every (b, joint, view, head):
 *   loc_p   = anchor[b,view,joint] + offs[b,joint,head,p] / (wid, hgt)
 *   a_p     = softmax_p(logits[b,joint,head,:])
 *   S_p(.)  = mmcv bilinear sample at pixel = loc*size - 0.5, zero padding
 *   g       = sum_p a_p S_p(feat[view,b])       (cf channels, all channels: the value projection is applied later)
 *   e       = sum_p a_p S_p(pos[view][:, head*dh:(head+1)*dh])   (optional, pos may be NULL)
 *   sigma   = sum_p a_p * (in-bounds bilinear weight mass)
 * Rows are ordered (b, joint, view) so that the projected result is already the concatenation
 * over views the fuse layer consumes.  rowmask[(b,joint,view)] = valid[b,view,joint].
 * offs_logits: (b*joint, heads*P*2 + heads*P) — offsets then attention logits (P = 16 points).
 */
int egr_msda_gather_f32(const float* feat /* (views, b, hgt*wid, cf) */, int32_t cf,
                        const float* pos /* (views, hgt*wid, heads*dh) or NULL */, int32_t dh,
                        const float* offs_logits, const float* anchors /* (b, views, joints, 2) */,
                        const uint8_t* valid /* (b, views, joints) */,
                        int32_t b, int32_t views, int32_t joints, int32_t heads, int32_t hgt, int32_t wid,
                        float* g /* (rows, heads, cf) */, float* e /* (rows, heads*dh) or NULL */,
                        float* sigma /* (heads, rows) */, uint8_t* rowmask /* (rows) */,
                        int32_t groups /* query sets sharing feat/anchors/valid: pos, offs_logits, g, e, sigma are [groups][...] */,
                        void* stream);

/*
 * One joint-query transformer layer behind its deformable sampling, as ONE launch (egr_layer.hip).  Replaces, per layer of
 * MultiViewTransformerLayer (egoposeformer_heatmap_mvf_ex.py:874-935) / EgoPoseFormerTransformerLayer
 * (egoposeformer_mvf_ex.py:546-588): MSDeformAttn's value / output projections on the sampled rows
 * (models/utils/deform_attn.py:122-168, sample-then-project form) with masked_fill(~valid), the concatenation over views +
 * fuse_mlp + residual + norm_cross, SpatialMHA (q/k/v/out projections and the softmax core, models/utils/transformer.py:36-93)
 * + residual + norm_spatial, FFN (transformer.py:8-33, exact-erf GELU) + residual + norm_ffn.  Optional tails: the NEXT layer's
 * sampling_offsets / attention_weights Linear on the new tokens, post_norm (heatmap_mvf_ex.py:707 / mvf_ex.py:411), and the
 * 3-D regression head reg_mlp + init anchors (mvf_ex.py:255-262, 412-418).
 * Operands: every weight is a plain row-major (groups, out, in) fp32 stack in the reference's Linear layout, biases / affine
 * parameters (groups, out).  g / e / sigma / rowmask are egr_msda_gather_f32's outputs; x the layer input (groups*b*joints, c).
 *   w_fold (groups, c, cf) = value_proj.weight . W_pre   (W_pre: the 1x1 conv in front of the attention), rows in head order
 *   c_fold (groups, c)     = value_proj.weight . b_pre + value_proj.bias       (scaled by sigma per row: zero padding)
 * Limits: views = 4, heads = 4, cf = 128, ffn_dim = 512, c in {128, 256}, joints <= 16; 16-byte aligned weights.
 */
typedef struct egr_layer_desc {
    int32_t B, J, V, C, heads, cf, groups, ffn_dim;
    float eps, mha_scale;                              /* LayerNorm eps (1e-5); softmax scale = (c / heads)^-1/2 */
    const float *x, *g, *e /* or NULL */, *sigma;
    const uint8_t* rowmask;
    const float *w_fold, *c_fold, *w_out, *b_out, *w_fuse, *b_fuse, *ln1_g, *ln1_b;
    const float *w_qkv, *b_qkv, *w_mo, *b_mo, *ln2_g, *ln2_b, *w_f0, *b_f0, *w_f1, *b_f1, *ln3_g, *ln3_b;
    float* x_out;                                      /* (groups*b*joints, c) */
    /* tail: next layer's offsets / logits (NULL = off): ol_out (groups*b*joints, ol_n), ol_n % 16 == 0 */
    const float *w_ol, *b_ol;
    float* ol_out;
    int32_t ol_n;
    int32_t w_packed;   /* != 0: every weight MATRIX (w_fold, w_out, w_fuse, w_qkv, w_mo, w_f0, w_f1, w_ol, w_r0; not w_r2, not the vectors) is in
                         * the fragment order of egr_pack_layer_w_f32 (1: fp32, 1-KiB contiguous wave loads) or of egr_pack_layer_wh2_f32
                         * (2: the fp16 scheme - two fp16 planes per weight, rows * k + rows floats per matrix, the contractions on
                         * v_mfma_f32_16x16x32_f16 with three products; what the shipped path passes under EGR_W_FORMAT=f16x2) */
    /* tail: post_norm (lnp_g NULL = off) -> xn_out (or NULL); with it the regression head: w_r0 (groups, c, c), w_r2 (groups, 3, c),
     * pred_out (groups*b*joints, 3) = reg(xn) + anchors3d */
    const float *lnp_g, *lnp_b;
    float* xn_out;
    const float *w_r0, *b_r0, *w_r2, *b_r2, *anchors3d;
    float* pred_out;
    /* tail (round 5): the refiner's head offset behind post_norm (heatmap_mvf_ex.py:707-711; TransformerHeadLayer.head[0..2]): the
     * (joints, c) tokens read as an s x s image (s * s == c; c = 256) with the joints as channels -> Conv2d(joints, h0_n, 1) + ReLU ->
     * Upsample(x2, bilinear, align_corners=True) -> h0_out (groups*b, 2s, 2s, h0_n) NHWC.  w_h0 (groups, h0_n, joints) plain
     * row-major, b_h0 (groups, h0_n); h0_n == 64; excludes the regression head.  amax_h0: NULL or the 64-slot abs-max record of
     * h0_out (receives an upper bound).  Replaces egr_tokens_to_nhwc_f32 + egr_linear_smallk_f32 + egr_upsample2x_nhwc_f32. */
    const float *w_h0, *b_h0;
    float* h0_out;
    uint32_t* amax_h0;
    int32_t h0_n;
} egr_layer_desc;
int egr_joint_layer_f32(const egr_layer_desc* d, void* stream);
/* Which kernel egr_joint_layer_f32 launches under w_packed = 2 (round 5): 1 (default; EGR_LAYER_PLANES) = every tile that feeds a
 * contraction is split ONCE into fragment-ordered fp16 planes in LDS, 0 = the round-4 kernel that splits inside the product loop;
 * bit-identical results.  on < 0 only queries.  Returns the previous setting. */
int egr_layer_set_planes(int on);
/* The JQA query of a refiner as ONE launch (round 5; HeatmapMVF.forward_feat_only, egoposeformer_heatmap_mvf_ex.py:655-665, behind
 * heatmap_proj[0] + ReLU):  hm_embed = heatmap_proj[2](t);  bfb = fc_bfb(adaptive_avg_pool2d(backbone_feat_bottom, (1, 1)));
 * x = ReLU(fc_query((joint_query_embed + bfb) + hm_embed));  ol = [sampling_offsets | attention_weights](x) of the refiner's
 * transformer layer (models/utils/deform_attn.py:122-135).  One workgroup per (query set, frame).
 * t (groups*b*joints, c); s32 (groups*b, pool_hw, kb) NHWC; embed (groups, joints, c); matrices w_hp2 (c, c), w_bfb (c, kb),
 * w_q (c, c), w_ol (ol_n, c) per group in the order w_packed names (egr_layer_desc.w_packed), vectors plain.
 * Limits: c = 256, kb = 512, joints <= 16, ol_n % 16 == 0.  Replaces egr_avgpool_nhwc_f32, egr_jqa_sum_f32 and four small
 * egr_conv2d_nhwc_f32 launches. */
typedef struct egr_jqa_query_desc {
    int32_t B, J, C, groups, kb, pool_hw, ol_n, w_packed;
    const float *t, *s32;
    const float *w_hp2, *b_hp2, *w_bfb, *b_bfb, *embed, *w_q, *b_q, *w_ol, *b_ol;
    float *x_out /* (groups*b*joints, c) */, *ol_out /* (groups*b*joints, ol_n) */;
} egr_jqa_query_desc;
int egr_jqa_query_f32(const egr_jqa_query_desc* d, void* stream);

/* The lifting head between mlp_pred[1] and its first decoder layer as ONE launch (round 5; egoposeformer_mvf_ex.py:255-262,
 * 317-322, 340-348, 400-410): pred = mlp_pred[2](h1) (b, joints, 3); the fisheye reprojection of egr_fisheye_project2_f32
 * (anchors3d_out = the points behind it: mutated in syn mode (ctm NULL), a copy in rw mode); x = query_gen_mlp([(j+1)/joints,
 * point]) (Linear(4, c) + ReLU, Linear + ReLU, Linear); ol = the first layer's [sampling_offsets | attention_weights](x).
 * One workgroup per frame.  h1 (b, c) = GELU(mlp_pred[1](..)); w_m2 (3*joints, c), w_qg2 / w_qg4 (c, c), w_ol (ol_n, c) in the
 * order w_packed names; w_qg0 (c, 4) and all vectors plain; cams / ctm as in egr_fisheye_project_f32.
 * Limits: c = 128, joints = 16, ol_n % 16 == 0.  Replaces egr_fisheye_project_f32, egr_linear_smallk_f32 and four small
 * egr_conv2d_nhwc_f32 launches. */
typedef struct egr_pose_query_desc {
    int32_t B, J, C, ol_n, w_packed;
    const float *h1, *w_m2, *b_m2, *ctm /* or NULL */, *cams;
    const float *w_qg0, *b_qg0, *w_qg2, *b_qg2, *w_qg4, *b_qg4, *w_ol, *b_ol;
    float *pred_out /* (b, joints, 3) */, *anchors3d_out /* (b, joints, 3) */, *anchors2d_out /* (b, 4, joints, 2) */;
    uint8_t* valid_out /* (b, 4, joints) */;
    float *x_out /* (b*joints, c) */, *ol_out /* (b*joints, ol_n) */;
} egr_pose_query_desc;
int egr_pose_query_f32(const egr_pose_query_desc* d, void* stream);

/* `matrices` row-major (rows, k) fp32 matrices (rows % 16 == 0, k % 128 == 0) -> the fragment order egr_joint_layer_f32 reads with
 * w_packed: [matrix][16-row block][128-deep chunk][16-deep k block u][lane = 16 q + i][4 floats] = w[16 block + i][128 chunk + 16 u + 4 q ..+3].
 * Same number of elements; out must not alias w. */
int egr_pack_layer_w_f32(const float* w, int32_t matrices, int32_t rows, int32_t k, float* out, void* stream);
/* The fp16-scheme image of the same matrices (w_packed = 2): per matrix rows * k + rows floats - [16-row block][128-deep chunk]
 * [32-deep k block][plane h | l][lane = 16 q + i][8 fp16] = plane of w[16 block + i][128 chunk + 32 kb + 8 q ..+7] * 2^e(row), then the
 * rows' descales 2^-e (fp32; e puts the row's largest magnitude into [2^14, 2^15), clamped to +-60).  Same limits as above. */
int egr_pack_layer_wh2_f32(const float* w, int32_t matrices, int32_t rows, int32_t k, float* out, void* stream);

/* utils/camera_models.py:53-104 + egoposeformer_mvf_ex.py:340-348,400-406: project the (b, joints, 3) proposals
 * into the four fisheye cameras.  cams: 4 records [npoly, cx, cy, W, H, poly[12]] (fp32).  syn mode
 * (ctm == NULL) reproduces the reference's in-place offset chain: `pts` is updated in place to the
 * mutated anchors.  rw mode applies ctm (b, 4, 4, 4) to pts*0.01 and scales by 100, pts untouched.
 * Also emits the decoder query input q4 = [ (joint+1)/joints, mutated pts ] (b, joints, 4). */
int egr_fisheye_project_f32(float* pts, const float* ctm, const float* cams, int32_t b, int32_t joints,
                            float* anchors /* (b, 4, joints, 2) */, uint8_t* valid /* (b, 4, joints) */,
                            float* q4, void* stream);
/* The same with the updated points written to pts_out (b, joints, 3) instead of in place: the mutated anchors in syn mode, a
 * copy of pts in rw mode - `init_anchors_3d = mlp_pred.clone()` (egoposeformer_mvf_ex.py:400) without the copy. */
int egr_fisheye_project2_f32(const float* pts, float* pts_out, const float* ctm, const float* cams, int32_t b, int32_t joints,
                             float* anchors, uint8_t* valid, float* q4, void* stream);

/* Small dense layer for K not a multiple of 32 (query_gen_mlp.0: K=4; head 1x1 conv: K=15):
 * y[m, n] = act(sum_k x[m*sxm + k*sxk] * w[n*K + k] + bias[n]). */
int egr_linear_smallk_f32(const float* x, int64_t sxm, int64_t sxk, const float* w, const float* bias, float* y,
                          int32_t m, int32_t n, int32_t k, int32_t act,
                          int32_t rows_per_group /* w + (row/rows_per_group)*n*k, bias + ..*n; 0 = one group */, void* stream);

/* JQA query pre-activation (heatmap_mvf_ex.py:664-665): y[b,j,:] = hm_embed[b,j,:] + embed[j,:] + bfb[b,:]. */
int egr_jqa_sum_f32(const float* hm_embed, const float* embed, const float* bfb, float* y,
                    int32_t b, int32_t j, int32_t c, int32_t b_per_group /* embed + (b/b_per_group)*j*c; 0 = one group */,
                    void* stream);

/* (b, j, s*s) token matrix -> NHWC (b, s, s, j) image with joints as channels (heatmap_mvf_ex.py:707-711). */
int egr_tokens_to_nhwc_f32(const float* x, float* y, int32_t b, int32_t j, int32_t hw, void* stream);

/* Frame pre-processing, replaces PIL.Image.resize([ow,oh], BICUBIC) + ToTensor + Normalize of
 * datasets/ego4view_syn/ego4view_syn_pose3d.py:41-44,159-162: src (n, h, w, 3) uint8 -> dst (n, 3, oh, ow) fp32.
 * bounds_* (out, 2) [first tap, tap count] and coef_* (out, ksize) 22-bit fixed-point weights are Pillow's
 * precompute_coeffs / normalize_coeffs_8bpc tables (host-computed); tmp (n, h, ow, 3) uint8 scratch;
 * mean / stdv: 3 HOST floats; u8out (n, oh, ow, 3) optional uint8 copy of the resized image (NULL to skip).
 * Alignment: tmp 4 bytes, dst 16 bytes, ow % 4 == 0 (EGR_EINVAL otherwise); src may sit at any byte address. */
int egr_preprocess_u8_f32(const uint8_t* src, int32_t n, int32_t h, int32_t w, int32_t oh, int32_t ow,
                          const int32_t* bounds_h, const int32_t* coef_h, int32_t ksize_h,
                          const int32_t* bounds_v, const int32_t* coef_v, int32_t ksize_v,
                          const float* mean, const float* stdv, uint8_t* tmp, float* dst, uint8_t* u8out, void* stream);
/* diagnostic (tests): the kernel of the last successful launch - 0 LDS horizontal pass, 1 aligned-dword, 2 generic, 3 fused. */
int egr_preprocess_last_kernel(void);

/* The same conversion as ONE launch: the horizontally resized uint8 rows of a 32-output-row band stay in LDS (no intermediate in
 * HBM, no `tmp`).  band_rows = egr_preprocess_band_rows(host copy of bounds_v, oh).  Returns EGR_EINVAL without launching when the
 * shape does not meet the kernel's limits (ow == 256, ksize_h <= 16, h % 4 == 0, 16-byte aligned rows-of-four, band in LDS): the
 * caller then falls back to egr_preprocess_u8_f32.  Bit-identical results. */
int egr_preprocess_band_rows(const int32_t* bounds_v_host, int32_t oh);
int egr_preprocess_fused_u8_f32(const uint8_t* src, int32_t n, int32_t h, int32_t w, int32_t oh, int32_t ow,
                                const int32_t* bounds_h, const int32_t* coef_h, int32_t ksize_h,
                                const int32_t* bounds_v, const int32_t* coef_v, int32_t ksize_v, int32_t band_rows,
                                const float* mean, const float* stdv, float* dst, uint8_t* u8out, void* stream);

/* Pose evaluation metrics per sample, replaces evaluate_pose of
 * pl_wrappers/egoposeformer/pose_3d_mvf_ex.py:317-333 (utils/loss.py:9-48, models/utils/pose_metric.py:104-167):
 * pred, gt (b, joints, 3) fp32 in cm -> out (b, 4) = [MPJPE mm, PA-MPJPE mm (similarity-aligned), PCK@pck_thr_mm %,
 * AUC % over n_auc thresholds linspace(0, pck_thr_mm, n_auc)]; aligned (b, joints, 3) optional (NULL to skip). */
int egr_pose_metrics_f32(const float* pred, const float* gt, int32_t b, int32_t joints, float pck_thr_mm, int32_t n_auc,
                         float* out, float* aligned, void* stream);

/* Ground-truth heat maps, replaces generate_target of generate_heatmap.py:10-48:
 * joints (maps, 2) float64 pixel coordinates in the image_size frame -> out (maps, heatmap_size, heatmap_size) fp32 with a
 * (2*tmp_size+1)^2 Gaussian window `gauss` (host table) centred on int(x * heatmap_size / image_size + 0.5). */
int egr_gt_heatmap_f32(const double* joints, int32_t maps, double image_size, int32_t heatmap_size, int32_t tmp_size,
                       const float* gauss, float* out, void* stream);

/* Heat-map validation metrics, replaces `evaluate` of pl_wrappers/egoposeformer/heatmap.py:220-254 and
 * heatmap_mvf_ex.py:263-316 (with get_max_preds, utils/loss.py:122-142, threshold heatmap_mvf_ex.py:308-310) and
 * `evaluate_heatmap` of pose_3d_mvf_ex.py:335-361 - a host loop with one device-to-host copy per sample there.
 *   preds: HOST array of `sets` (1..EGR_HM_MAX_SETS) device pointers, each (b, v, joints, hgt, wid) fp32 dense, as is gt, which is
 *   read once for all sets; view_groups: HOST array of n_groups (1..EGR_HM_MAX_GROUPS) pairs [v0, v1), 0 <= v0 < v1 <= v.
 * Per map (work / by-products): partials (sets, b*v*joints, 3) fp64 = {sum |p-g|, the same where g > 0, sum (p-g)^2};
 * argmax (sets + 1, b*v*joints) flat index of the first maximum and maxval (sets + 1, b*v*joints), row `sets` = the ground
 * truth; valid (b*v*joints) = [max(gt) >= threshold].
 * Per set and view group: l1, pos_l1 (sets, n_groups, b) per-sample sums over the group's views and all positions; mse
 * (sets, n_groups) = mean of (p-g)^2; mse_pts2d (sets, n_groups) = mean over (b, group views, joints, 2) of
 * (pts(p) * valid - pts(g) * valid)^2 with pts = (index % wid, index / wid).
 * Sums accumulate in fp64 in a fixed order (no atomics): two calls on the same inputs give the same bits.  Two launches on
 * `stream`, no synchronisation, no allocation.  EGR_EINVAL: hgt*wid not a multiple of 4, joints > 32, too many sets / groups,
 * an empty or out-of-range view group, a pointer that is not 16-byte aligned. */
#define EGR_HM_MAX_SETS 4
#define EGR_HM_MAX_GROUPS 8
int egr_heatmap_metrics_f32(const float* const* preds, int32_t sets, const float* gt, int32_t b, int32_t v, int32_t joints,
                            int32_t hgt, int32_t wid, const int32_t* view_groups, int32_t n_groups, float threshold,
                            double* partials, int32_t* argmax, float* maxval, uint8_t* valid, float* l1, float* pos_l1,
                            float* mse, float* mse_pts2d, void* stream);

/* The reference's only native call, in its own operand layout: mmcv==2.2.0 MultiScaleDeformableAttnFunction.apply
 * (models/utils/deform_attn.py:155-162; third-party, un-vendored, pin README.md:134).
 *   value (n, lin, heads, d) fp32, spatial_shapes i64 (levels, 2) = (H_l, W_l), level_start_index i64 (levels) — both
 *   device arrays —, sampling_loc (n, lq, heads, levels, points, 2) normalised (x, y), attn_weight (n, lq, heads, levels,
 *   points)  ->  out (n, lq, heads*d).
 * pixel = loc*size - 0.5; a point contributes iff -1 < pixel < size on both axes; corners outside the map read as 0.
 * im2col_step of the reference only chunks the batch and has no counterpart here.  Corner tokens >= lin are skipped, so
 * inconsistent shapes cannot fault.  The model path itself uses egr_msda_gather_f32 (sample-then-project); these two
 * entries serve a maintainer who replaces only the mmcv extension (egorear_amd/msda.py). */
int egr_msda_fwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const float* sampling_loc, const float* attn_weight, int32_t n, int64_t lin, int32_t heads, int32_t d,
                     int32_t lq, int32_t levels, int32_t points, float* out, void* stream);
/* Backward of the above: grad_value (n, lin, heads, d) is zeroed on the stream and then accumulated with atomics (the
 * summation order, and so the last bits, vary run to run — as in mmcv); grad_sampling_loc and grad_attn_weight are
 * written for every point (zeros for points outside the map). */
int egr_msda_bwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const float* sampling_loc, const float* attn_weight, const float* grad_out, int32_t n, int64_t lin,
                     int32_t heads, int32_t d, int32_t lq, int32_t levels, int32_t points, float* grad_value,
                     float* grad_sampling_loc, float* grad_attn_weight, void* stream);

/* Library / device identification. */
const char* egr_version(void);
int egr_device_arch(char* buf, int32_t buflen); /* gcnArchName of the current device */

#ifdef __cplusplus
}
#endif
#endif /* EGOREAR_HIP_H */
