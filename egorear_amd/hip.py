"""ctypes binding of libegorear_hip.so (C ABI: include/egorear_hip.h).

PyTorch is used here only as the owner of device memory and streams: every wrapper
takes torch tensors, checks device / dtype / layout on the host (a kernel fault can
reset the GPU), extracts raw pointers and the current HIP stream, and calls the C
entry point.  There is no fallback: if the library is missing, import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from typing import Optional, Union

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EGR_LIB") or os.path.join(_HERE, "csrc", "libegorear_hip.so")   # EGR_LIB: experiment builds (tools/build_variant.py)

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
RES_NONE, RES_BEFORE_ACT, RES_AFTER_ACT, RES_UP2_BEFORE_ACT = 0, 1, 2, 3


# --------------------------------------------------------------------------- launch policy

import contextlib
import dataclasses
import sys
import types


class _on_default:
    """A method that also answers on the class, for the default policy: LaunchPolicy.fast() is LaunchPolicy().fast()."""

    def __init__(self, fn):
        self.fn = fn
        self.__doc__ = fn.__doc__

    def __get__(self, obj, cls):
        return types.MethodType(self.fn, obj if obj is not None else cls())


@dataclasses.dataclass
class LaunchPolicy:
    """Which kernel family a launch goes to - ONE object instead of module globals (round 6).  A module (engine.set_policy) or a
    caller (`with hip.use_policy(p):`, thread-local) can hold its own; everything else follows the process default `hip.POLICY`,
    which is made from the environment at import.  The historical module attributes (hip.H2, hip.X6_MIN_ROWS, hip.CHAIN_*,
    engine.W_FORMAT, engine.LAYER_H2, engine.FUSED_*) are properties onto it: reading one returns the ACTIVE policy's value,
    assigning one changes the process default (what the parity tests that sweep launch rules do)."""
    # weight operand of the implicit-GEMM launches: "f16x2" = bf16x3 image + fp16 companion, "bf16x3", "f32" (engine._w_operand);
    # "f16" = the operands of "f16x2" with the one-product bit on the conv launches (fast(), opt-in: outside the parity contract)
    w_format: str = "f16x2"
    # the fp16 scheme for the launches whose input carries an abs-max record (EGR_W_FORMAT=bf16x3 / f32 switch it off)
    h2: bool = True
    # Below these sizes (all groups together) a launch is bound by latency or by streaming the weights once, not by the matrix
    # cores: it keeps the 4-byte weight format (measured: 3840 rows x K 4096 slower with the split, 8192 rows x N 512 x K 4608
    # faster).  Re-swept with the tap-sharing / streaming kernels in place (tools/x6_small_sweep.sh: 8192 rows / 4e9 flops ->
    # 4096 / 5e8: batch 2-16 latency -2 .. -7 %, batch 32 +1.9 % frames/s, batch 1 and 64 unchanged)
    x6_min_rows: int = 4096
    x6_min_flops: float = 5e8
    # the training step keeps the rule its gradient goldens were recorded under (tests/test_gpu_train_step.py; train.py passes x6_min)
    x6_train_min_rows: int = 8192
    x6_train_min_flops: float = 4e9
    # two 1x1 convolutions back to back as one launch (egr_conv1x1_chain_f32): EGR_CONV_CHAIN=0 keeps the pair of launches
    chain: bool = True
    chain_min_rows: int = 8192       # (measured: batch 1 1.46 -> 1.41 ms with the FPN level-1 chain; smaller chains lose)
    chain_big: bool = True           # the streamed 256 -> 256 -> 128 form (conv_pw2_kernel)
    chain_big_min_rows: int = 65536
    # weight gradients of large layers on the 16-bit matrix cores with operand splits (the kernel keeps small ones on fp32 MFMA)
    wgrad_x6: bool = True
    wgrad_force: bool = False        # tests: every weight-gradient launch on the split kernel, whatever its size
    # engine: the fused transformer layer's contractions in the fp16 scheme; one launch per layer / per token chain
    layer_h2: bool = True
    fused_layer: bool = True
    fused_query: bool = True
    # engine: the refiners' up-sampled feature map ReLU(up2(y)) is produced by the lifting head's first 1x1 conv as it loads y
    # (egr_conv_aux.in_mode) instead of by a launch of its own; EGR_UP2_ON_LOAD=0 keeps the up-sampling launch
    up2_on_load: bool = True
    # the half-precision TRAINING arithmetic on top of w_format "f16" (fast_training(), opt-in: outside the parity contract): the training
    # step's role-split conv launches and its split weight gradients multiply fp16-rounded operands with one product
    train_one_product: bool = False

    @classmethod
    def from_env(cls, env=None) -> "LaunchPolicy":
        e = os.environ if env is None else env
        fmt = e.get("EGR_W_FORMAT", "f16x2")
        fp16 = fmt in ("f16x2", "f16")
        tfmt = e.get("EGR_TRAIN_FORMAT", "")
        if tfmt not in ("", "f16") or (tfmt == "f16" and fmt != "f16"):
            raise ValueError("egorear_amd: EGR_TRAIN_FORMAT=f16 is the only value, and it requires EGR_W_FORMAT=f16")
        return cls(train_one_product=tfmt == "f16", w_format=fmt, h2=fp16,
                   x6_min_rows=int(e.get("EGR_X6_MIN_ROWS", "4096")), x6_min_flops=float(e.get("EGR_X6_MIN_FLOPS", "5e8")),
                   x6_train_min_rows=int(e.get("EGR_X6_TRAIN_MIN_ROWS", "8192")), x6_train_min_flops=float(e.get("EGR_X6_TRAIN_MIN_FLOPS", "4e9")),
                   chain=e.get("EGR_CONV_CHAIN", "1") != "0", chain_min_rows=int(e.get("EGR_CONV_CHAIN_MIN_ROWS", "8192")),
                   chain_big=e.get("EGR_CONV_CHAIN_BIG", "1") != "0", chain_big_min_rows=int(e.get("EGR_CONV_CHAIN_BIG_MIN_ROWS", "65536")),
                   wgrad_x6=fmt != "f32", layer_h2=fp16 and e.get("EGR_LAYER_H2", "1") != "0",
                   fused_layer=e.get("EGR_FUSED_LAYER", "1") != "0", fused_query=e.get("EGR_FUSED_QUERY", "1") != "0",
                   up2_on_load=e.get("EGR_UP2_ON_LOAD", "1") != "0")

    def replace(self, **kw) -> "LaunchPolicy":
        return dataclasses.replace(self, **kw)

    def pack_key(self) -> tuple:
        """The fields that shape packed weights and abs-max arenas (engine.State, train.PackCache): packs made under one key are not
        valid under another."""
        key = (self.w_format, self.h2, self.layer_h2)
        # (the training mode adds an element instead of widening every key: a captured step replays the launches it recorded, one-product
        # ones included, so a cache made under fast_training() is not fast()'s - and the keys of all other policies stay what they were)
        return key + ("train_f16",) if self.train_one_product else key

    def exact(self) -> "LaunchPolicy":
        """The exact-operand arithmetic (EGR_W_FORMAT=bf16x3): three bf16 planes, six products, fused layers on the fp32 matrix cores."""
        return self.replace(w_format="bf16x3", h2=False, layer_h2=False)

    @_on_default
    def fast(self) -> "LaunchPolicy":
        """The half-precision serving arithmetic (EGR_W_FORMAT=f16), opt-in and outside the parity contract: the forward launches of the
        role-split conv kernel multiply the fp16 scheme's HIGH planes only - fp16-rounded operands, one matrix product instead of
        three, fp32 accumulation (EGR_W_F16X1).  Same packs and records as "f16x2" (made again under this policy's own
        pack_key); every launch without a one-product kernel - stem, chains, fused layers, weight stream, small launches - runs what
        it runs under the default policy.  The training step ignores the bit: it computes what it computes under "f16x2" (its own
        half-precision mode is fast_training())."""
        return self.replace(w_format="f16", h2=True, layer_h2=True)

    @_on_default
    def fast_training(self) -> "LaunchPolicy":
        """fast() plus the half-precision TRAINING arithmetic (EGR_W_FORMAT=f16 EGR_TRAIN_FORMAT=f16), opt-in and outside the parity
        contract: the training step's role-split conv launches - statistics epilogue, masked and plain stride-1 data gradients
        (EGR_W_F16X1T) - and its split weight gradients (EGR_W_F16X1 on egr_conv2d_wgrad_ex_f32) multiply the HIGH fp16 planes only,
        one product, fp32 accumulation.  Master weights, optimizer, BatchNorm and every launch without a one-product
        kernel are what they are under the default policy; no loss scaling (every operand is pre-scaled from its abs-max record)."""
        return self.fast().replace(train_one_product=True)

    @property
    def fp16_scheme(self) -> bool:
        """The weight format carries the fp16 companion images ("f16x2", or "f16" on top of it)."""
        return self.w_format in ("f16x2", "f16")


POLICY = LaunchPolicy.from_env()       # the process default
_POLICY_TLS = threading.local()


def policy() -> LaunchPolicy:
    """The policy in force for the calling thread: the innermost `use_policy`, else the process default."""
    cur = getattr(_POLICY_TLS, "cur", None)
    return cur if cur is not None else POLICY


@contextlib.contextmanager
def use_policy(p: Optional[LaunchPolicy]):
    """Launches issued by this thread inside the block follow `p` (None: no change)."""
    if p is None:
        yield
        return
    old = getattr(_POLICY_TLS, "cur", None)
    _POLICY_TLS.cur = p
    try:
        yield
    finally:
        _POLICY_TLS.cur = old


def install_policy_properties(module_name: str, mapping: dict) -> None:
    """{MODULE_ATTRIBUTE: LaunchPolicy field}: the module's historical knobs become properties - read = the active policy, write =
    the process default."""
    def make(field):
        return property(lambda self: getattr(policy(), field), lambda self, v: setattr(POLICY, field, v))
    mod = sys.modules[module_name]
    mod.__class__ = type("_PolicyModule", (types.ModuleType,), {name: make(field) for name, field in mapping.items()})


install_policy_properties(__name__, {
    "H2": "h2", "X6_MIN_ROWS": "x6_min_rows", "X6_MIN_FLOPS": "x6_min_flops", "X6_TRAIN_MIN_ROWS": "x6_train_min_rows",
    "X6_TRAIN_MIN_FLOPS": "x6_train_min_flops", "CHAIN": "chain", "CHAIN_MIN_ROWS": "chain_min_rows", "CHAIN_BIG": "chain_big",
    "CHAIN_BIG_MIN_ROWS": "chain_big_min_rows", "WGRAD_X6": "wgrad_x6", "WGRAD_FORCE": "wgrad_force"})

EXPORTS = [
    "egr_conv2d_nhwc_f32", "egr_stem_conv7x7_f32", "egr_maxpool_nhwc_f32", "egr_upsample2x_nhwc_f32",
    "egr_avgpool_nhwc_f32", "egr_argmax_rows_f32", "egr_layernorm_f32", "egr_joint_mha_f32", "egr_msda_gather_f32",
    "egr_fisheye_project_f32", "egr_linear_smallk_f32", "egr_jqa_sum_f32", "egr_tokens_to_nhwc_f32", "egr_version",
    "egr_device_arch", "egr_conv_force_config", "egr_preprocess_u8_f32", "egr_pose_metrics_f32", "egr_gt_heatmap_f32", "egr_conv_debug_stamps", "egr_conv2d_wgrad_f32", "egr_conv2d_masked_f32", "egr_up2_relu_head_f32",
    "egr_msda_fwd_f32", "egr_msda_bwd_f32", "egr_w6_elems", "egr_pack_w6_f32", "egr_pack_w6_many_f32", "egr_joint_layer_f32",
    "egr_preprocess_fused_u8_f32", "egr_preprocess_band_rows", "egr_preprocess_last_kernel", "egr_conv_set_persist", "egr_stem_conv7x7_pool_f32",
    "egr_stem_w6_bytes", "egr_pack_stem_w6_f32", "egr_stem_conv7x7_x6_f32", "egr_wgrad_last_kernel", "egr_conv_last_kernel", "egr_conv_set_tap", "egr_conv_set_tapx", "egr_conv_set_splitk_fused", "egr_fisheye_project2_f32", "egr_pack_layer_w_f32", "egr_pack_layer_wh2_f32",
    "egr_conv2d_nhwc_ex_f32", "egr_wh2_elems", "egr_pack_wh2_f32", "egr_absmax_f32", "egr_stem_conv7x7_x6_ex_f32", "egr_stem_wh2_bytes", "egr_pack_stem_wh2_f32", "egr_stem_conv7x7_h2_f32",
    "egr_pack_wh2_many_f32", "egr_conv2d_masked_ex_f32", "egr_conv2d_wgrad_ex_f32", "egr_wgrad_last_h2", "egr_wgrad_last_planes",
    "egr_wstream_image_bytes", "egr_pack_wstream_f32", "egr_linear_wstream_workspace_bytes", "egr_linear_wstream_f32", "egr_conv1x1_chain_f32",
    "egr_jqa_query_f32", "egr_pose_query_f32", "egr_layer_set_planes", "egr_head_set_persist", "egr_heatmap_metrics_f32",
    "egr_conv_plan", "egr_soft_argmax_f32", "egr_soft_argmax_bwd_f32", "egr_coord_l1_f32",
    "egr_triangulate_f32", "egr_triangulate_bwd_f32", "egr_volume_fuse_f32", "egr_volume_fuse_bwd_f32",
    "egr_peaks_f32", "egr_consensus_f32", "egr_skeleton_fit_f32", "egr_bone_lengths_f32", "egr_skeleton_resize_f32",
    "egr_trajectory_smooth_f32", "egr_trajectory_smooth_bwd_f32", "egr_rig_refine_f32", "egr_rig_refine_workspace_bytes",
    "egr_ray_track_f32", "egr_ray_track_workspace_bytes",
    "egr_joint_info_f32", "egr_info_track_f32", "egr_info_track_workspace_bytes",
    "egr_trajectory_filter_state_slots", "egr_trajectory_filter_f32", "egr_trajectory_filter_tail_f32",
]


class NMap(C.Structure):
    _fields_ = [("n_inner", C.c_int32), ("stride_inner", C.c_int64), ("stride_outer", C.c_int64)]


class ConvDesc(C.Structure):
    _fields_ = [
        ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("ho", C.c_int32), ("wo", C.c_int32), ("ldx", C.c_int32), ("ldy", C.c_int32), ("ldr", C.c_int32),
        ("xmap", NMap), ("ymap", NMap), ("rmap", NMap),
        ("act", C.c_int32), ("res_mode", C.c_int32), ("out_nchw", C.c_int32), ("split_k", C.c_int32),
        ("groups", C.c_int32),
        ("gx", C.c_int64), ("gw", C.c_int64), ("gp", C.c_int64), ("gy", C.c_int64), ("gr", C.c_int64),
        ("grs", C.c_int64), ("grm", C.c_int64),
        ("transposed", C.c_int32), ("w_format", C.c_int32),
    ]


class ConvAux(C.Structure):
    """egr_conv_aux of include/egorear_hip.h: side operands of the fp16 scheme (EGR_W_F16X2) and the abs-max record of the output."""
    _fields_ = [("w_descale", C.c_void_p), ("amax_in", C.c_void_p), ("amax_out", C.c_void_p),
                ("bn_partials", C.c_void_p), ("bn_tiles_out", C.c_void_p), ("bn_capacity", C.c_int64),
                ("in_mode", C.c_int32), ("in_up2_out", C.c_void_p)]


IN_PLAIN, IN_UP2_RELU = 0, 1      # egr_conv_aux.in_mode


class ConvPlan(C.Structure):
    """egr_conv_plan_t of include/egorear_hip.h: what a conv launch will do (route, tile, variant, grid, split-K, ...)."""
    _fields_ = [(n, C.c_int32) for n in ("route", "bm", "bn", "variant", "planes", "tiles_m", "tiles_n", "grid_x", "grid_y", "grid_z", "block",
                                         "split_k", "ktiles_per_split", "persistent", "cls_mode", "fused_reduce", "reduce_pass", "bn_slabs")]


# egr_conv_route: the values of ConvPlan.route and of conv_last_kernel()
ROUTE_F32_TILED, ROUTE_SPLIT_TILED, ROUTE_TAP, ROUTE_TAP2, ROUTE_STREAM_1X1, ROUTE_SMALL_F32, ROUTE_TAPX = range(7)
# the values of egr_preprocess_last_kernel(): which horizontal-pass kernel (or the fused one) the last successful call launched
PRE_ROUTE_LDS, PRE_ROUTE_DWORD, PRE_ROUTE_GENERIC, PRE_ROUTE_FUSED = range(4)
# egr_conv_desc.w_format bits the wrappers set by name (include/egorear_hip.h)
W_F16X2, W_F16X1, W_F16X1T = 4, 8, 16


class ChainAux(C.Structure):
    """egr_chain_aux of include/egorear_hip.h: the second conv of egr_conv1x1_chain_f32."""
    _fields_ = [("w2", C.c_void_p), ("w2_descale", C.c_void_p), ("shift1", C.c_void_p), ("cmid", C.c_int32), ("act1", C.c_int32),
                ("gw2", C.c_int64), ("gp1", C.c_int64)]


class LayerDesc(C.Structure):
    """egr_layer_desc of include/egorear_hip.h (field for field)."""
    _P = C.c_void_p
    _fields_ = ([(n, C.c_int32) for n in ("B", "J", "V", "C", "heads", "cf", "groups", "ffn_dim")] +
                [("eps", C.c_float), ("mha_scale", C.c_float)] +
                [(n, C.c_void_p) for n in ("x", "g", "e", "sigma", "rowmask",
                                           "w_fold", "c_fold", "w_out", "b_out", "w_fuse", "b_fuse", "ln1_g", "ln1_b",
                                           "w_qkv", "b_qkv", "w_mo", "b_mo", "ln2_g", "ln2_b", "w_f0", "b_f0", "w_f1", "b_f1", "ln3_g", "ln3_b",
                                           "x_out", "w_ol", "b_ol", "ol_out")] +
                [("ol_n", C.c_int32), ("w_packed", C.c_int32)] +
                [(n, C.c_void_p) for n in ("lnp_g", "lnp_b", "xn_out", "w_r0", "b_r0", "w_r2", "b_r2", "anchors3d", "pred_out",
                                           "w_h0", "b_h0", "h0_out", "amax_h0")] +
                [("h0_n", C.c_int32)])


class JqaQueryDesc(C.Structure):
    """egr_jqa_query_desc of include/egorear_hip.h (field for field)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "J", "C", "groups", "kb", "pool_hw", "ol_n", "w_packed")] +
                [(n, C.c_void_p) for n in ("t", "s32", "w_hp2", "b_hp2", "w_bfb", "b_bfb", "embed", "w_q", "b_q", "w_ol", "b_ol",
                                           "x_out", "ol_out")])


class PoseQueryDesc(C.Structure):
    """egr_pose_query_desc of include/egorear_hip.h (field for field)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "J", "C", "ol_n", "w_packed")] +
                [(n, C.c_void_p) for n in ("h1", "w_m2", "b_m2", "ctm", "cams", "w_qg0", "b_qg0", "w_qg2", "b_qg2", "w_qg4", "b_qg4",
                                           "w_ol", "b_ol", "pred_out", "anchors3d_out", "anchors2d_out", "valid_out", "x_out", "ol_out")])


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m egorear_amd.csrc.build` "
            "(or __graft_entry__.build()).  egorear_amd has no CPU / PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.egr_conv2d_nhwc_f32.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.egr_conv2d_nhwc_ex_f32.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(ConvAux), vp]
    lib.egr_conv_plan.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(ConvAux), C.POINTER(ConvPlan)]
    lib.egr_conv1x1_chain_f32.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, C.POINTER(ConvAux), C.POINTER(ChainAux), vp]
    lib.egr_fill_f32.argtypes = [vp, f32, i64, vp]      # (include/egorear_train.h; zeroes the abs-max records)
    lib.egr_fill_f32.restype = C.c_int
    lib.egr_absmax_f32.argtypes = [vp, i64, vp, vp]
    lib.egr_wh2_elems.restype = C.c_int64
    lib.egr_wh2_elems.argtypes = [i32, i32]
    lib.egr_pack_wh2_f32.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.egr_stem_conv7x7_f32.argtypes = [vp, NMap, i32, i32, i32, vp, vp, vp, vp, i32, i64, vp]
    lib.egr_stem_conv7x7_pool_f32.argtypes = [vp, NMap, i32, i32, i32, vp, vp, vp, vp, i32, i64, vp]
    lib.egr_wgrad_last_kernel.argtypes = []
    lib.egr_wgrad_last_planes.argtypes = []
    lib.egr_conv_last_kernel.argtypes = []
    lib.egr_conv_set_tap.argtypes = [i32]
    lib.egr_conv_set_tapx.argtypes = [i32, i32, i32]
    lib.egr_conv_set_splitk_fused.argtypes = [i32]
    lib.egr_stem_w6_bytes.restype = C.c_int64
    lib.egr_stem_w6_bytes.argtypes = []
    lib.egr_pack_stem_w6_f32.argtypes = [vp, i32, vp, vp]
    lib.egr_stem_conv7x7_x6_f32.argtypes = [vp, NMap, i32, i32, i32, vp, vp, vp, vp, i32, i32, i64, vp]
    lib.egr_stem_conv7x7_x6_ex_f32.argtypes = [vp, NMap, i32, i32, i32, vp, vp, vp, vp, i32, i32, i64, vp, vp]
    lib.egr_stem_wh2_bytes.restype = C.c_int64
    lib.egr_stem_wh2_bytes.argtypes = []
    lib.egr_pack_stem_wh2_f32.argtypes = [vp, i32, vp, vp, vp]
    lib.egr_stem_conv7x7_h2_f32.argtypes = [vp, NMap, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, i64, vp, vp]
    lib.egr_wstream_image_bytes.restype = C.c_int64
    lib.egr_wstream_image_bytes.argtypes = [i32, i32]
    lib.egr_pack_wstream_f32.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.egr_linear_wstream_workspace_bytes.restype = C.c_int64
    lib.egr_linear_wstream_workspace_bytes.argtypes = [i32, i32, i32]
    lib.egr_linear_wstream_f32.argtypes = [vp, i64, i32, i32, vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, i64, vp]
    lib.egr_maxpool_nhwc_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.egr_upsample2x_nhwc_f32.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.egr_avgpool_nhwc_f32.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.egr_argmax_rows_f32.argtypes = [vp, i32, i32, i32, f32, vp, vp, vp, vp, vp]
    lib.egr_soft_argmax_f32.argtypes = [vp, i32, i32, i32, f32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp]
    lib.egr_soft_argmax_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, i32, vp, vp]
    lib.egr_triangulate_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp]
    lib.egr_triangulate_bwd_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp]
    lib.egr_volume_fuse_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp]
    lib.egr_volume_fuse_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp]
    lib.egr_peaks_f32.argtypes = [vp, i32, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp]
    lib.egr_consensus_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, i32, f32, vp, vp, vp, vp, vp, vp, vp]
    lib.egr_skeleton_fit_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, f32, f32, f32, f32, f32, f32, i32, vp, vp, vp, vp,
                                         vp, vp, vp, vp, vp]
    lib.egr_bone_lengths_f32.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.egr_skeleton_resize_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.egr_trajectory_smooth_f32.argtypes = [vp, vp, vp, i32, i32, i32, f32, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.egr_trajectory_smooth_bwd_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp]
    lib.egr_trajectory_filter_state_slots.restype = C.c_int64
    lib.egr_trajectory_filter_state_slots.argtypes = [i32]
    lib.egr_trajectory_filter_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, i32, vp, vp, vp, vp, vp, vp]
    lib.egr_trajectory_filter_tail_f32.argtypes = [vp, i32, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp]
    lib.egr_rig_refine_workspace_bytes.restype = C.c_int64
    lib.egr_rig_refine_workspace_bytes.argtypes = [i32, i32, i32]
    lib.egr_rig_refine_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, i32, f32, i32, vp, i64, vp, vp, vp, vp, vp, vp,
                                       vp, vp, vp, vp]
    lib.egr_ray_track_workspace_bytes.restype = C.c_int64
    lib.egr_ray_track_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.egr_ray_track_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, f32, i32, i32, C.c_double, vp, i64, vp, vp, vp,
                                      vp, vp, vp, vp]
    lib.egr_joint_info_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp]
    lib.egr_info_track_workspace_bytes.restype = C.c_int64
    lib.egr_info_track_workspace_bytes.argtypes = [i32, i32, i32]
    lib.egr_info_track_f32.argtypes = [vp, vp, vp, i32, i32, i32, f32, f32, f32, i32, i32, C.c_double, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.egr_coord_l1_f32.argtypes = [vp, vp, vp, i32, i32, f32, vp, vp, vp]
    lib.egr_layernorm_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, f32, i32, vp]
    lib.egr_joint_mha_f32.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp]
    lib.egr_msda_gather_f32.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.egr_fisheye_project_f32.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.egr_fisheye_project2_f32.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.egr_linear_smallk_f32.argtypes = [vp, i64, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.egr_jqa_sum_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.egr_tokens_to_nhwc_f32.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.egr_version.restype = C.c_char_p
    lib.egr_w6_elems.restype = C.c_int64
    lib.egr_device_arch.argtypes = [C.c_char_p, i32]
    lib.egr_conv_force_config.argtypes = [i32]
    lib.egr_conv_set_persist.argtypes = [i32, i32]
    lib.egr_up2_relu_head_f32.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, vp, i32, i64, i64, i32, i64, vp]
    lib.egr_conv2d_masked_f32.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.egr_conv2d_masked_ex_f32.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(ConvAux), vp]
    lib.egr_conv2d_wgrad_f32.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, C.c_size_t, i32, vp]
    lib.egr_conv2d_wgrad_ex_f32.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, C.c_size_t, i32, vp, vp, vp]
    lib.egr_gt_heatmap_f32.argtypes = [vp, i32, C.c_double, i32, i32, vp, vp, vp]
    lib.egr_pose_metrics_f32.argtypes = [vp, vp, i32, i32, f32, i32, vp, vp, vp]
    lib.egr_heatmap_metrics_f32.argtypes = [C.POINTER(vp), i32, vp, i32, i32, i32, i32, i32, C.POINTER(i32), i32, f32,
                                            vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.egr_pack_w6_f32.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.egr_pack_w6_many_f32.argtypes = [vp, i32, i64, vp]
    lib.egr_pack_wh2_many_f32.argtypes = [vp, i32, i64, i64, vp]
    lib.egr_w6_elems.argtypes = [i32, i32]
    lib.egr_msda_fwd_f32.argtypes = [vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, vp, vp]
    lib.egr_msda_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.egr_joint_layer_f32.argtypes = [C.POINTER(LayerDesc), vp]
    lib.egr_jqa_query_f32.argtypes = [C.POINTER(JqaQueryDesc), vp]
    lib.egr_pose_query_f32.argtypes = [C.POINTER(PoseQueryDesc), vp]
    lib.egr_pack_layer_w_f32.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.egr_pack_layer_wh2_f32.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.egr_preprocess_fused_u8_f32.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.egr_preprocess_band_rows.argtypes = [vp, i32]
    lib.egr_preprocess_last_kernel.argtypes = []
    lib.egr_preprocess_u8_f32.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    for name in EXPORTS:
        getattr(lib, name)  # fail at import if a symbol is missing
        if name not in ("egr_version", "egr_w6_elems", "egr_stem_w6_bytes", "egr_wh2_elems", "egr_stem_wh2_bytes", "egr_wstream_image_bytes",
                        "egr_linear_wstream_workspace_bytes", "egr_rig_refine_workspace_bytes",
                        "egr_ray_track_workspace_bytes", "egr_info_track_workspace_bytes"):
            getattr(lib, name).restype = C.c_int
    return lib


lib = _load()

_ERR = {-1: "EGR_EINVAL (unsupported shape/alignment)", -2: "EGR_ENULL (missing pointer)", -3: "EGR_EWORKSPACE"}


class LaunchError(RuntimeError):
    """A C-ABI entry point returned non-zero: `code` is its return value (-1 EGR_EINVAL, -2 EGR_ENULL, -3 EGR_EWORKSPACE, > 0 a
    hipError_t), so that a caller with a second way to run the launch can tell "this shape is not supported here" from a device fault."""

    def __init__(self, name: str, code: int):
        super().__init__(f"{name} failed: {_ERR.get(code, 'hipError_t %d' % code)}")
        self.name, self.code = name, code


EINVAL, ENULL, EWORKSPACE = -1, -2, -3


def _check(rc: int, name: str):
    if rc != 0:
        raise LaunchError(name, rc)


# When PROFILE is a list, every launch is bracketed by HIP events recorded on the launch stream (torch's current
# stream) and (kernel name, start, end, algorithmic work) is appended; bench.py uses this for the roofline leg.
PROFILE = None
# When PLAN_LOG is a list, every conv2d launch (the masked data gradients too) first asks egr_conv_plan what it is about to launch and appends
# (tag, ConvPlan): which launches of a forward took which route / variant / plane count (tests, tools/fast_bench.py).
PLAN_LOG = None


# Device of the launch being assembled: set by the first tensor handed to _p(), checked for every further one, consumed by
# _launch().  The kernel goes to the current stream OF THAT DEVICE (not of torch's current device), and the C entry point is called
# with that device current - a module on cuda:1 works while torch.cuda.current_device() is 0 (two replicas in one process, a caller
# that never called set_device).
# Per Python thread (two replicas may be driven by two threads: the ctypes call releases the GIL between _p() and _launch());
# every path out of a launch - success, a host-side validation error, a failed call - leaves it cleared.
class _Dev(threading.local):
    idx = None


_DEVL = _Dev()


class _DevSlot:
    """_DEV[0] of earlier versions, now backed by the thread-local record."""

    def __getitem__(self, _i):
        return _DEVL.idx

    def __setitem__(self, _i, v):
        _DEVL.idx = v


_DEV = _DevSlot()


def _launch(name: str, cfunc, *args, flops: float = 0.0, nbytes: float = 0.0, tag: str = ""):
    idx, _DEV[0] = _DEV[0], None
    if idx is not None and idx != torch.cuda.current_device():
        with torch.cuda.device(idx):
            return _launch_here(name, cfunc, args, flops, nbytes, tag)
    return _launch_here(name, cfunc, args, flops, nbytes, tag)


def _launch_here(name, cfunc, args, flops, nbytes, tag):
    if PROFILE is None:
        rc = cfunc(*args)
    else:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = cfunc(*args)
        e.record()
        PROFILE.append((name, s, e, flops, nbytes, tag))
    _check(rc, name)


def _p(t: Optional[torch.Tensor], dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        _DEV[0] = None
        raise RuntimeError("egorear_amd: tensor is not on a HIP device (no CPU path exists)")
    if t.dtype != dtype:
        _DEV[0] = None
        raise RuntimeError(f"egorear_amd: expected {dtype}, got {t.dtype}")
    idx = t.device.index
    if _DEV[0] is None:
        _DEV[0] = idx
    elif _DEV[0] != idx:
        first, _DEV[0] = _DEV[0], None
        raise RuntimeError(f"egorear_amd: operands of one launch live on different devices (cuda:{first} and cuda:{idx})")
    return C.c_void_p(t.data_ptr())


def _pv(t: Optional[torch.Tensor]):
    """Raw device pointer of a tensor of any dtype (same device bookkeeping as _p)."""
    return None if t is None else _p(t, t.dtype)


def _stream():
    """Current stream of the device the launch's tensors live on (falls back to torch's current device for tensor-less calls)."""
    idx = _DEV[0] if _DEV[0] is not None else torch.cuda.current_device()
    return C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)


def _cont(t: torch.Tensor, what: str):
    if not t.is_contiguous():
        raise RuntimeError(f"egorear_amd: {what} must be contiguous")
    return t


def version() -> str:
    return lib.egr_version().decode()


def conv_force_config(cfg: int):
    _check(lib.egr_conv_force_config(cfg), "egr_conv_force_config")


def conv_set_persist(slots: int = -1, max_ktiles: int = -1):
    _check(lib.egr_conv_set_persist(slots, max_ktiles), "egr_conv_set_persist")


def conv_plan(d: "ConvDesc", x, w, y, *, scale=None, shift=None, res=None, rowscale=None, rowmask=None, mask=None, workspace=None,
              workspace_floats: int = 0, aux: Optional["ConvAux"] = None):
    """(return code, ConvPlan) of egr_conv_plan: what egr_conv2d_nhwc_ex_f32 (mask None) / egr_conv2d_masked_ex_f32 would launch for
    these arguments.  Operands are raw addresses (ints or None): none is dereferenced and no device is touched."""
    out = ConvPlan()
    rc = lib.egr_conv_plan(C.byref(d), x, w, scale, shift, res, rowscale, rowmask, mask, y, workspace, workspace_floats,
                           C.byref(aux) if aux is not None else None, C.byref(out))
    return rc, out


def device_arch() -> str:
    buf = C.create_string_buffer(256)
    _check(lib.egr_device_arch(buf, 256), "egr_device_arch")
    return buf.value.decode()


# --------------------------------------------------------------------------- NHWC views

class Img:
    """A batch of channels-last images living (possibly as a channel slice) in a torch buffer.
    t: (N, H, W, C) with stride(3) == 1 and dense H/W (stride(1) == W*ld, stride(2) == ld)."""
    __slots__ = ("t", "n", "h", "w", "c", "ld", "nstride", "amax")

    def __init__(self, t: torch.Tensor, amax: Optional[torch.Tensor] = None):
        if t.dim() != 4 or t.stride(3) != 1:
            raise RuntimeError("egorear_amd: expected a channels-last (N,H,W,C) tensor")
        n, h, w, c = t.shape
        ld = t.stride(2) if w > 1 else (t.stride(1) if h > 1 else max(c, 1))
        if (w > 1 and h > 1 and t.stride(1) != w * ld):
            raise RuntimeError("egorear_amd: image rows must be dense")
        self.t, self.n, self.h, self.w, self.c, self.ld = t, n, h, w, c, ld
        self.nstride = t.stride(0) if n > 1 else h * w * ld
        # abs-max record of the tensor (64 uint32 slots, see egr_conv2d_nhwc_ex_f32) or None: left by the launch that produced it,
        # carried by the tensor object, read by a consuming EGR_W_F16X2 launch
        self.amax = amax if amax is not None else getattr(t, "_egr_amax", None)

    def tag(self, amax: Optional[torch.Tensor]):
        """Attach (or clear) the abs-max record: every launch that writes the tensor calls this."""
        self.amax = amax
        self.t._egr_amax = amax

    def nmap(self) -> NMap:
        return NMap(self.n, self.nstride, 0)


# --------------------------------------------------------------------------- ops

class W6:
    """Packed weights in the EGR_W_BF16X3 format (egr_pack_w6_f32): every fp32 weight as hi + mid + lo bf16, in fragment
    order.  Passed to conv2d in place of the packed fp32 matrix, it selects the bf16-matrix-core launch."""
    __slots__ = ("img", "npad", "K", "groups", "gstride", "f32", "used", "h2", "h2_ds", "h2_gstride", "h2_used")

    def __init__(self, img, npad, K, groups, gstride, f32=None):
        self.img, self.npad, self.K, self.groups, self.gstride = img, npad, K, groups, gstride
        self.f32 = f32      # the fp32 matrix it was made from: small launches stay on it (X6_MIN_ROWS / X6_MIN_FLOPS)
        self.used = False   # set by the first launch that takes the image (the training step only re-splits those)
        # EGR_W_F16X2 image of the same matrix (two fp16 planes of w * 2^k[co]) + the per-channel descale 2^-k[co]: taken by forward
        # launches whose input carries an abs-max record (add_wh2)
        self.h2 = self.h2_ds = None
        self.h2_gstride = 0
        self.h2_used = False    # set by the first launch that takes the fp16 image

    @property
    def shape(self):
        return (self.groups, self.npad, self.K) if self.groups > 1 else (self.npad, self.K)


def pack_w6(w: torch.Tensor) -> W6:
    """w: packed fp32 weights (npad, K) or (groups, npad, K) as conv2d takes them."""
    _cont(w, "packed weight")
    groups = w.shape[0] if w.dim() == 3 else 1
    npad, K = int(w.shape[-2]), int(w.shape[-1])
    n = int(lib.egr_w6_elems(npad, K))
    if n == 0:
        raise RuntimeError(f"egorear_amd.pack_w6: unsupported weight shape {tuple(w.shape)} (rows and K must be multiples of 32)")
    img = torch.empty(groups * n, device=w.device, dtype=torch.bfloat16)
    _launch("egr_pack_w6_f32", lib.egr_pack_w6_f32, _p(w), npad, K, groups, _p(img, torch.bfloat16), _stream())
    return W6(img, npad, K, groups, n, w)


def add_wh2(w6: W6) -> W6:
    """Give a W6 operand its EGR_W_F16X2 image (egr_pack_wh2_f32), made from the fp32 matrix it keeps."""
    if w6.f32 is None:
        raise RuntimeError("egorear_amd.add_wh2: the operand does not keep its fp32 matrix")
    n = int(lib.egr_wh2_elems(w6.npad, w6.K))
    img = torch.empty(w6.groups * n, device=w6.f32.device, dtype=torch.float16)
    ds = torch.empty(w6.groups * w6.npad, device=w6.f32.device, dtype=torch.float32)
    _launch("egr_pack_wh2_f32", lib.egr_pack_wh2_f32, _p(w6.f32), w6.npad, w6.K, w6.groups, _p(img, torch.float16), _p(ds), _stream())
    w6.h2, w6.h2_ds, w6.h2_gstride = img, ds, n
    return w6


ARENA_EXHAUSTED = 0      # over every AmaxArena of the process (bench.py reports it: a non-zero count means silent fallbacks)


class AmaxArena:
    """Abs-max records of one forward: 64 uint32 slots per recorded tensor in ONE buffer, zeroed by one launch when the forward
    begins (egr_fill_f32: all-zero bits), handed out in launch order.  A graph replay re-runs the fill and every producer."""

    def __init__(self, device, records: int = 256):
        self.buf = torch.zeros(records * 64, device=device, dtype=torch.int32)
        self.records, self.k = records, 0
        self.exhausted = 0        # requests refused since construction: each one is a launch that left the fp16 scheme

    def begin(self):
        self.k = 0
        _launch("egr_fill_f32", lib.egr_fill_f32, _p(self.buf, torch.int32), 0.0, self.buf.numel(), _stream())

    def new(self) -> Optional[torch.Tensor]:
        global ARENA_EXHAUSTED
        if self.k >= self.records:
            self.exhausted += 1
            ARENA_EXHAUSTED += 1
            return None
        self.k += 1
        return self.buf[(self.k - 1) * 64:self.k * 64]


def absmax_record(t: torch.Tensor, record: torch.Tensor) -> torch.Tensor:
    """Fold max |t| of a dense fp32 tensor into `record` (64 int32 slots, e.g. AmaxArena.new()) and tag the tensor with it: for
    tensors that enter the path from outside, so that their consumers can take the fp16 scheme."""
    _cont(t, "tensor")
    if record.numel() != 64 or record.dtype != torch.int32:
        raise RuntimeError("egorear_amd.absmax_record: the record is 64 int32 slots")
    _launch("egr_absmax_f32", lib.egr_absmax_f32, _p(t), t.numel(), _p(record, torch.int32), _stream(), nbytes=4.0 * t.numel())
    t._egr_amax = record
    return record


def pack_w6_into(w6: W6) -> None:
    """Refresh an image from its fp32 matrix (w6.f32) in place: the training step does this after every parameter update."""
    _launch("egr_pack_w6_f32", lib.egr_pack_w6_f32, _p(w6.f32), w6.npad, w6.K, w6.groups, _p(w6.img, torch.bfloat16), _stream())


class W6Job(C.Structure):
    _fields_ = [("w", C.c_void_p), ("img", C.c_void_p), ("npad", C.c_int32), ("k", C.c_int32), ("groups", C.c_int32), ("reserved", C.c_int32),
                ("first_block", C.c_int64)]


class W6Table:
    """Device table for egr_pack_w6_many_f32: every image of `images` re-split from its fp32 matrix in ONE launch."""

    def __init__(self, images):
        self.images = list(images)
        jobs = (W6Job * max(1, len(self.images)))()
        first = 0
        for i, w6 in enumerate(self.images):
            jobs[i] = W6Job(w6.f32.data_ptr(), w6.img.data_ptr(), w6.npad, w6.K, w6.groups, 0, first)
            first += w6.groups * ((w6.npad // 32 + 3) // 4 * 4) * (w6.K // 32)
        self.total = first
        raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).clone()
        self.dev = raw.to(self.images[0].img.device) if self.images else None

    def run(self):
        if self.images:
            _launch("egr_pack_w6_f32", lib.egr_pack_w6_many_f32, _p(self.dev, torch.uint8), len(self.images), self.total, _stream())


class WH2Job(C.Structure):
    _fields_ = [("w", C.c_void_p), ("img", C.c_void_p), ("descale", C.c_void_p), ("npad", C.c_int32), ("k", C.c_int32), ("groups", C.c_int32),
                ("reserved", C.c_int32), ("first_rblock", C.c_int64), ("first_pblock", C.c_int64)]


class WH2Table:
    """Device table for egr_pack_wh2_many_f32: the fp16 image (and descale) of every operand of `images` re-made from its fp32 matrix in
    two launches."""

    def __init__(self, images):
        self.images = list(images)
        jobs = (WH2Job * max(1, len(self.images)))()
        fr = fp = 0
        for i, w6 in enumerate(self.images):
            jobs[i] = WH2Job(w6.f32.data_ptr(), w6.h2.data_ptr(), w6.h2_ds.data_ptr(), w6.npad, w6.K, w6.groups, 0, fr, fp)
            fr += (w6.groups * w6.npad + 3) // 4
            fp += w6.groups * ((w6.npad // 32 + 3) // 4 * 4) * (w6.K // 32)
        self.rblocks, self.pblocks = fr, fp
        raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).clone()
        self.dev = raw.to(self.images[0].h2.device) if self.images else None

    def run(self):
        if self.images:
            _launch("egr_pack_wh2_f32", lib.egr_pack_wh2_many_f32, _p(self.dev, torch.uint8), len(self.images), self.rblocks, self.pblocks, _stream())


def pack_wh2_into(w6: W6) -> None:
    """Refresh the fp16 image of an operand from its fp32 matrix in place."""
    _launch("egr_pack_wh2_f32", lib.egr_pack_wh2_f32, _p(w6.f32), w6.npad, w6.K, w6.groups, _p(w6.h2, torch.float16), _p(w6.h2_ds), _stream())


def conv2d(x: Img, w, cout: int, kh: int, kw: int, stride: int, pad: int, *, scale=None, shift=None,
           act: int = ACT_NONE, res: Optional[Img] = None, res_mode: int = RES_NONE, rowscale=None, rowmask=None,
           out: Optional[Img] = None, out_nchw: Optional[torch.Tensor] = None, ymap: Optional[NMap] = None,
           xmap: Optional[NMap] = None, rmap: Optional[NMap] = None, workspace: Optional[torch.Tensor] = None,
           split_k: int = 1, groups: int = 1, gx: Optional[int] = None, gy: Optional[int] = None,
           gr: Optional[int] = None, grs: int = 0, grm: int = 0, transposed_out_hw: Optional[tuple] = None, x6_min: Optional[tuple] = None,
           mask: Optional[Img] = None, amax_out: Optional[torch.Tensor] = None, amax_arena: Optional["AmaxArena"] = None,
           bn_ws: Optional[torch.Tensor] = None, bn_slabs: Optional[list] = None, one_product: Union[bool, str, None] = None,
           up2_in: bool = False, up2_out: Optional[Img] = None) -> Optional[Img]:
    """Implicit-GEMM conv / linear.  Output goes to `out` (NHWC Img, maybe a channel slice), or to the raw
    tensor `out_nchw` (channel-major planes placed by `ymap`), or to a fresh NHWC tensor.

    groups > 1: `groups` same-shape problems in one launch.  w is (groups, cout_pad, K), scale/shift
    (groups, cout_pad).  x / out / res hold the images of all groups back to back (group stride = images per group x
    image stride) unless an explicit element stride gx / gy / gr is given, in which case they describe group 0.

    one_product: None = the policy's forward rule (w_format "f16"), True / False = EGR_W_F16X1 on / off (tests), "train" = the training
    step under LaunchPolicy.train_one_product: EGR_W_F16X1 | EGR_W_F16X1T, the role-split route's training launches take one product too.

    up2_in: x is the HALF-RESOLUTION tensor and the launch convolves ReLU(bilinear x2(x)), interpolated as it is loaded
    (egr_conv_aux.in_mode = EGR_IN_UP2_RELU; bit-identical to upsample2x(x, relu=True) followed by the plain launch); up2_out: a dense
    (groups * n, 2 h, 2 w, cin) Img that then also receives that operand.  Returns None - nothing launched - when the library has no
    kernel for the call in this mode (EGR_EINVAL from egr_conv_plan): the caller materialises the up-sampled tensor instead."""
    pol = policy()
    x_full = x.t
    if up2_in and (mask is not None or out_nchw is not None or transposed_out_hw is not None or bn_ws is not None or res_mode != RES_NONE):
        raise RuntimeError("egorear_amd.conv2d: up2_in goes with a plain NHWC forward launch only")
    if up2_out is not None and not up2_in:
        raise RuntimeError("egorear_amd.conv2d: up2_out without up2_in")
    if groups > 1:
        if gx is None:
            if x.n % groups:
                raise RuntimeError("egorear_amd.conv2d: images not divisible by groups")
            ng = x.n // groups
            gx = ng * x.nstride
            x = Img(x.t[:ng], amax=x.amax)
        ng = x.n
    ih, iw = (2 * x.h, 2 * x.w) if up2_in else (x.h, x.w)      # the image the conv runs over
    if transposed_out_hw is not None:   # data gradient: x is dy, the output is dx of the given spatial size
        ho, wo = transposed_out_hw
        if (ho + 2 * pad - kh) // stride + 1 != x.h or (wo + 2 * pad - kw) // stride + 1 != x.w:
            raise RuntimeError("egorear_amd.conv2d: transposed_out_hw inconsistent with dy's size")
    else:
        ho = (ih + 2 * pad - kh) // stride + 1
        wo = (iw + 2 * pad - kw) // stride + 1
    npad = (cout + 31) // 32 * 32
    K = kh * kw * x.c
    wshape = (groups, npad, K) if groups > 1 else (npad, K)
    if tuple(w.shape) != wshape:
        raise RuntimeError(f"egorear_amd.conv2d: packed weight shape {tuple(w.shape)} != {wshape}")
    if isinstance(w, W6) and w.f32 is not None:
        rows_all = x.n * groups * ho * wo
        # (the split kernel addresses one group's activations through a 2-GiB buffer window)
        x_bytes = 4 * ((x.n - 1) * x.nstride + (ih * iw + 2 * (kh * iw + kw + 1)) * x.ld) + 64
        min_rows, min_flops = x6_min if x6_min is not None else (pol.x6_min_rows, pol.x6_min_flops)
        if rows_all < min_rows or 2.0 * rows_all * cout * K < min_flops or x_bytes >= (1 << 31):
            w = w.f32
    x6 = isinstance(w, W6)
    if x6 and pol.h2 and w.h2 is not None and x.amax is None and amax_arena is not None and x_full.is_contiguous():
        # an input without a record (it comes out of a launch that keeps none): one read of it makes one (the training step)
        rec = amax_arena.new()
        if rec is not None:
            absmax_record(x_full, rec)
            x.amax = rec
    # the fp16 scheme: launches whose input carries its abs-max record (the launch's pre-scale comes from it)
    h2 = x6 and pol.h2 and w.h2 is not None and x.amax is not None
    if x6 and not h2 and not w.used:
        if w.f32 is not None:
            pack_w6_into(w)     # an owner that only re-splits the images in use (the training step) may have left this one stale
        w.used = True
    if h2 and not w.h2_used:
        if w.f32 is not None:
            pack_wh2_into(w)
        w.h2_used = True
    wptr = (_p(w.h2, torch.float16) if h2 else _p(w.img, torch.bfloat16)) if x6 else _p(_cont(w, "packed weight"))
    d = ConvDesc()
    d.w_format = (4 if h2 else 1) if x6 else 0
    # the fast policy (or one_product=True: tests): the same operands plus EGR_W_F16X1 - the dispatch takes a one-product kernel where
    # one exists (plan.planes == 1) and treats the bit as absent everywhere else
    h1 = h2 and (pol.w_format == "f16" if one_product is None else bool(one_product))
    h1t = h1 and one_product == "train"
    if h1:
        d.w_format |= W_F16X1 | (W_F16X1T if h1t else 0)
    d.n, d.h, d.w, d.cin, d.cout = x.n, ih, iw, x.c, cout
    d.kh, d.kw, d.stride, d.pad, d.ho, d.wo = kh, kw, stride, pad, ho, wo
    d.ldx = x.ld
    d.xmap = xmap if xmap is not None else x.nmap()
    if up2_in and not h2:
        return None                                    # (the mode exists in the fp16 scheme only: nothing launched)
    d.act, d.res_mode, d.split_k = act, res_mode, split_k
    d.transposed = 1 if transposed_out_hw is not None else 0
    d.groups, d.gx, d.gw, d.gp, d.grs, d.grm = groups, (gx or 0), (((w.h2_gstride if h2 else w.gstride) if x6 else npad * K) if groups > 1 else 0), (npad if groups > 1 else 0), grs, grm
    ret = None
    if out_nchw is not None:
        if ymap is None or (groups > 1 and gy is None):
            raise RuntimeError("egorear_amd.conv2d: out_nchw needs ymap (and gy when grouped)")
        d.out_nchw, d.ldy, d.ymap, d.gy = 1, 0, ymap, (gy or 0)
        yptr = _p(out_nchw)
    else:
        full = out
        if out is None:
            full = Img(torch.empty((groups * x.n, ho, wo, cout), device=x.t.device, dtype=torch.float32))
            out = full
        if groups > 1 and gy is None:
            if out.n != groups * x.n:
                raise RuntimeError("egorear_amd.conv2d: grouped output must hold groups x n images")
            gy = x.n * out.nstride
            out = Img(out.t[:x.n])
        if (out.n, out.h, out.w, out.c) != (x.n, ho, wo, cout) and ymap is None:
            raise RuntimeError(f"egorear_amd.conv2d: output shape {(out.n, out.h, out.w, out.c)} != {(x.n, ho, wo, cout)}")
        d.out_nchw, d.ldy, d.gy = 0, out.ld, (gy or 0)
        d.ymap = ymap if ymap is not None else out.nmap()
        yptr = _p(out.t)
        ret = full
    if res_mode != RES_NONE:
        if res is None:
            raise RuntimeError("egorear_amd.conv2d: res_mode set without res")
        if groups > 1 and gr is None:
            if res.n != groups * x.n:
                raise RuntimeError("egorear_amd.conv2d: grouped residual must hold groups x n images")
            gr = x.n * res.nstride
            res = Img(res.t[:x.n])
        if res_mode == RES_UP2_BEFORE_ACT and (2 * res.h != ho or 2 * res.w != wo or res.c < cout):
            raise RuntimeError("egorear_amd.conv2d: the upsampled residual must be exactly half the output resolution")
        d.ldr, d.gr = res.ld, (gr or 0)
        d.rmap = rmap if rmap is not None else res.nmap()
    else:
        d.rmap = NMap(1, 0, 0)
    for t, nm in ((scale, "scale"), (shift, "shift")):
        if t is not None and t.numel() < (groups * npad if groups > 1 else cout):
            raise RuntimeError(f"egorear_amd.conv2d: {nm} shorter than expected")
    M = x.n * ho * wo
    if rowscale is not None and rowscale.numel() < (groups - 1) * grs + M or rowmask is not None and rowmask.numel() < (groups - 1) * grm + M:
        raise RuntimeError("egorear_amd.conv2d: rowscale/rowmask shorter than M")
    ws_ptr, ws_n = (None, 0) if workspace is None else (_p(workspace), workspace.numel())
    if mask is not None:   # output *= [mask > 0]; mask has the output's dense layout
        if out_nchw is not None or scale is not None or shift is not None or rowscale is not None or rowmask is not None or act != ACT_NONE:
            raise RuntimeError("egorear_amd.conv2d: mask goes with a plain NHWC data gradient only")
        if (mask.n, mask.h, mask.w, mask.c) != (groups * x.n, ho, wo, cout) or not mask.t.is_contiguous() or ret is None or not ret.t.is_contiguous():
            raise RuntimeError("egorear_amd.conv2d: mask must be dense and shaped like the output")
        if amax_out is not None and (amax_out.numel() != 64 or amax_out.dtype != torch.int32 or not amax_out.is_contiguous()):
            raise RuntimeError("egorear_amd.conv2d: amax_out must be 64 contiguous int32 slots")
        aux = None
        if h2 or amax_out is not None:
            aux = ConvAux(_p(w.h2_ds).value if h2 else None, _p(x.amax, torch.int32).value if h2 else None,
                          _p(amax_out, torch.int32).value if amax_out is not None else None)
        ret.tag(amax_out)
        x6 = x6 and not h2     # (the tag below)
        fmt = "h2 " if h2 else ""
        if PLAN_LOG is not None or (h1t and PROFILE is not None):
            dev, plan = _DEV[0], ConvPlan()
            _check(lib.egr_conv_plan(C.byref(d), _p(x.t), wptr, None, None, _p(res.t) if res is not None else None, None, None, _p(mask.t),
                                     yptr, ws_ptr, ws_n, C.byref(aux) if aux is not None else None, C.byref(plan)), "egr_conv_plan")
            _DEV[0] = dev
            fmt = "h1 " if plan.planes == 1 else fmt       # (the tag says what the launch multiplies)
            if PLAN_LOG is not None:
                PLAN_LOG.append((f"{fmt}masked G{groups} M{M} N{cout} K{K} k{kh}s{stride} cin{x.c}", plan))
        _launch("egr_conv2d_nhwc_f32", lib.egr_conv2d_masked_ex_f32, C.byref(d), _p(x.t), wptr, _p(res.t) if res is not None else None,
                _p(mask.t), yptr, ws_ptr, ws_n, C.byref(aux) if aux is not None else None, _stream(),
                flops=2.0 * M * cout * K * groups / (stride * stride if transposed_out_hw is not None else 1),
                nbytes=4.0 * groups * (2 * M * cout + x.n * x.h * x.w * x.c + cout * K),
                tag=f"{'T ' if transposed_out_hw is not None else ''}{fmt}{'x6 ' if x6 else ''}masked G{groups} M{M} N{cout} K{K} k{kh}s{stride} cin{x.c}" if PROFILE is not None else "")
        return ret
    if out_nchw is not None:
        amax_out = None          # (the channel-major epilogue keeps no record)
    elif amax_out is not None and (amax_out.numel() != 64 or amax_out.dtype != torch.int32 or not amax_out.is_contiguous()):
        raise RuntimeError("egorear_amd.conv2d: amax_out must be 64 contiguous int32 slots")
    aux = None
    tiles = None
    if h2 or amax_out is not None or bn_ws is not None:
        aux = ConvAux(_p(w.h2_ds).value if h2 else None, _p(x.amax, torch.int32).value if h2 else None,
                      _p(amax_out, torch.int32).value if amax_out is not None else None, None, None, 0)
        if bn_ws is not None:
            # train-mode BatchNorm behind this conv: the launch leaves the per-tile channel statistics in `bn_ws` (float64 workspace of
            # hip_train.bn_workspace) and reports its slab count in bn_slabs[0] (egr_conv_aux.bn_partials)
            if bn_ws.dtype != torch.float64 or bn_slabs is None:
                raise RuntimeError("egorear_amd.conv2d: bn_ws is the float64 BatchNorm workspace, bn_slabs a list receiving the slab count")
            tiles = C.c_int32(0)
            aux.bn_partials = _p(bn_ws, torch.float64).value
            aux.bn_tiles_out = C.addressof(tiles)
            aux.bn_capacity = bn_ws.numel()
    if up2_in:
        if up2_out is not None and ((up2_out.n, up2_out.h, up2_out.w, up2_out.c) != (groups * x.n, ih, iw, x.c) or not up2_out.t.is_contiguous()):
            raise RuntimeError("egorear_amd.conv2d: up2_out must be a dense (groups * n, 2 h, 2 w, cin) tensor")
        aux.in_mode = IN_UP2_RELU
        aux.in_up2_out = _p(up2_out.t).value if up2_out is not None else None
        # decided on the host first: a call the library has no kernel for in this mode launches nothing
        dev, probe = _DEV[0], ConvPlan()
        rc = lib.egr_conv_plan(C.byref(d), _p(x.t), wptr, _p(scale), _p(shift), None, _p(rowscale), _p(rowmask, torch.uint8), None, yptr,
                               ws_ptr, ws_n, C.byref(aux), C.byref(probe))
        _DEV[0] = dev
        if rc == EINVAL:
            return None
        _check(rc, "egr_conv_plan")
    fmt = ("h1 " if h1 else "h2 ") if h2 else ("x6 " if x6 else "")
    if PLAN_LOG is not None or (h1t and PROFILE is not None):
        dev, plan = _DEV[0], ConvPlan()
        _check(lib.egr_conv_plan(C.byref(d), _p(x.t), wptr, _p(scale), _p(shift), _p(res.t) if res is not None else None, _p(rowscale),
                                 _p(rowmask, torch.uint8), None, yptr, ws_ptr, ws_n, C.byref(aux) if aux is not None else None, C.byref(plan)),
               "egr_conv_plan")
        _DEV[0] = dev
        if h1t:                                        # the training step: the tag says what the launch multiplies
            fmt = "h1 " if plan.planes == 1 else "h2 "
        if PLAN_LOG is not None:
            PLAN_LOG.append((f"{fmt}G{groups} M{M} N{cout} K{K} k{kh}s{stride} cin{x.c}", plan))
    _launch("egr_conv2d_nhwc_f32", lib.egr_conv2d_nhwc_ex_f32, C.byref(d), _p(x.t), wptr, _p(scale), _p(shift),
            _p(res.t) if res is not None else None, _p(rowscale), _p(rowmask, torch.uint8), yptr, ws_ptr, ws_n,
            C.byref(aux) if aux is not None else None, _stream(),
            flops=2.0 * M * cout * K * groups / (stride * stride if transposed_out_hw is not None else 1),
            nbytes=4.0 * groups * (M * cout + x.n * x.h * x.w * x.c + cout * K + (M * x.c if up2_out is not None else 0)),
            tag=f"{'T ' if transposed_out_hw is not None else ''}{fmt}G{groups} M{M} N{cout} K{K} k{kh}s{stride} cin{x.c}" if PROFILE is not None else "")
    if up2_out is not None:
        up2_out.tag(x.amax)    # bilinear interpolation (+ ReLU) is a convex combination: the input's record bounds it (as upsample2x)
    if ret is not None:
        ret.tag(amax_out)      # (also clears a stale record when this launch keeps none)
    if tiles is not None:
        bn_slabs[:] = [int(tiles.value)]
    return ret


def chain_eligible(x: Img, w1, w2, cmid: int, cout: int, groups: int, scale1=None, scale2=None, res_mode: int = 0) -> bool:
    """Whether conv1x1_chain covers this pair: fp16 scheme on both operands, x carries its abs-max record, cin 64 / 128 -> 128 -> <= 128,
    bias-only convs, enough pixels for the streaming structure (the rule of the single streaming launches)."""
    pol = policy()
    if not (pol.chain and pol.h2 and isinstance(w1, W6) and isinstance(w2, W6) and w1.h2 is not None and w2.h2 is not None):
        return False
    if x.amax is None or scale1 is not None or scale2 is not None or cout > 128 or cout % 4:
        return False
    big = x.c == 256 and cmid == 256        # both matrices streamed through LDS (conv_pw2_kernel: the heat-map heads' 256 -> 256 -> 128)
    if not big and (x.c not in (64, 128) or cmid != 128):
        return False
    if big and (not pol.chain_big or res_mode != RES_NONE):
        return False
    if x.n % groups or w1.groups != groups or w2.groups != groups or w1.npad != cmid or w2.npad != 128 or w1.K != x.c or w2.K != cmid:
        return False
    # the entry's own layout checks (egr_conv1x1_chain_f32 returns EINVAL on them): 16-byte pixel rows and image strides, a 16-byte
    # aligned base - a channel slice at an odd offset stays on the single launches instead of aborting the forward
    if x.ld % 4 or x.nstride % 4 or x.t.data_ptr() % 16:
        return False
    return x.n * x.h * x.w >= (pol.chain_big_min_rows if big else pol.chain_min_rows)


def conv1x1_chain(x: Img, w1, w2, cmid: int, cout: int, *, shift1=None, shift2=None, act1: int = ACT_RELU, act2: int = ACT_NONE,
                  res: Optional[Img] = None, res_mode: int = RES_NONE, out: Optional[Img] = None, groups: int = 1,
                  amax_out: Optional[torch.Tensor] = None) -> Img:
    """y = act2(W2 . act1(W1 . x + shift1) + shift2 [+ res]) in one launch; the cmid-channel intermediate never reaches memory.
    x / out / res hold the images of all groups back to back (as hip.conv2d).  Call chain_eligible first."""
    if not chain_eligible(x, w1, w2, cmid, cout, groups, res_mode=res_mode):
        raise LaunchError("egr_conv1x1_chain_f32", EINVAL)
    ng = x.n // groups
    gx = ng * x.nstride if groups > 1 else 0
    xg = Img(x.t[:ng], amax=x.amax) if groups > 1 else x
    for w in (w1, w2):
        if not w.h2_used:
            if w.f32 is not None:
                pack_wh2_into(w)
            w.h2_used = True
    d = ConvDesc()
    d.w_format = 4
    d.n, d.h, d.w, d.cin, d.cout = xg.n, xg.h, xg.w, xg.c, cout
    d.kh, d.kw, d.stride, d.pad, d.ho, d.wo = 1, 1, 1, 0, xg.h, xg.w
    d.ldx, d.xmap = xg.ld, xg.nmap()
    d.act, d.res_mode, d.split_k, d.transposed, d.out_nchw = act2, res_mode, 1, 0, 0
    full = out
    if out is None:
        full = Img(torch.empty((x.n, x.h, x.w, cout), device=x.t.device, dtype=torch.float32))
        out = full
    if out.n != x.n or (out.h, out.w, out.c) != (x.h, x.w, cout):
        raise RuntimeError("egorear_amd.conv1x1_chain: output shape does not match")
    gy = ng * out.nstride if groups > 1 else 0
    og = Img(out.t[:ng]) if groups > 1 else out
    d.ldy, d.ymap = og.ld, og.nmap()
    gr = 0
    if res_mode != RES_NONE:
        if res is None or res.n != x.n:
            raise RuntimeError("egorear_amd.conv1x1_chain: res_mode set without a residual of groups x n images")
        if res_mode == RES_UP2_BEFORE_ACT and (2 * res.h != x.h or 2 * res.w != x.w or res.c < cout):
            raise RuntimeError("egorear_amd.conv1x1_chain: the upsampled residual must be exactly half the output resolution")
        gr = ng * res.nstride if groups > 1 else 0
        rg = Img(res.t[:ng]) if groups > 1 else res
        d.ldr, d.rmap = rg.ld, rg.nmap()
    else:
        d.rmap = NMap(1, 0, 0)
    d.groups, d.gx, d.gw, d.gp, d.gy, d.gr = groups, gx, (w1.h2_gstride if groups > 1 else 0), (128 if groups > 1 else 0), gy, gr
    for t, nm, need, gs in ((shift1, "shift1", cmid, w1.npad), (shift2, "shift2", cout, 128)):
        if t is not None and t.numel() < ((groups - 1) * gs + need):
            raise RuntimeError(f"egorear_amd.conv1x1_chain: {nm} shorter than expected")
    if amax_out is not None and (amax_out.numel() != 64 or amax_out.dtype != torch.int32 or not amax_out.is_contiguous()):
        raise RuntimeError("egorear_amd.conv1x1_chain: amax_out must be 64 contiguous int32 slots")
    aux = ConvAux(_p(w1.h2_ds).value, _p(x.amax, torch.int32).value, _p(amax_out, torch.int32).value if amax_out is not None else None, None, None, 0)
    ch = ChainAux(_p(w2.h2, torch.float16).value, _p(w2.h2_ds).value, _p(shift1).value if shift1 is not None else None, cmid, act1,
                  (w2.h2_gstride if groups > 1 else 0), (w1.npad if groups > 1 else 0))
    M = ng * x.h * x.w
    _launch("egr_conv1x1_chain_f32", lib.egr_conv1x1_chain_f32, C.byref(d), _p(xg.t), _p(w1.h2, torch.float16), _p(shift2),
            _p(res.t) if res is not None else None, _p(og.t), C.byref(aux), C.byref(ch), _stream(),
            flops=2.0 * M * groups * (cmid * x.c + cout * cmid), nbytes=4.0 * groups * (M * (cout + x.c) + cmid * x.c + cout * cmid),
            tag=f"h2 chain G{groups} M{M} N{cout} K{x.c} k1s1 cin{x.c} mid{cmid}" if PROFILE is not None else "")
    full.tag(amax_out)
    return full


def wgrad_records(x: Img, dy: Img, amax_arena: Optional["AmaxArena"]) -> None:
    """Abs-max records for the operands of a split weight-gradient launch that carry none (one read each), on the current stream."""
    if not policy().h2 or amax_arena is None:
        return
    for im in (x, dy):
        if im.amax is None and im.t.is_contiguous():
            rec = amax_arena.new()
            if rec is not None:
                absmax_record(im.t, rec)
                im.amax = rec


def conv2d_wgrad(x: Img, dy: Img, kh: int, kw: int, stride: int, pad: int, workspace: torch.Tensor, *, want_bias: bool = False,
                 dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None, accumulate: bool = False, groups: int = 1,
                 x6: Optional[bool] = None, amax_arena: Optional["AmaxArena"] = None, gx: Optional[int] = None, gy: Optional[int] = None,
                 one_product: Optional[bool] = None):
    """Weight (+ bias) gradient of the forward conv x -> y.  x, dy NHWC Imgs (all groups' images back to back when
    groups > 1).  Returns (dw, db): dw ([groups,] cout, kh*kw*cin) in the packed K order of conv2d
    (engine.unpack_conv_weight turns it back into OIHW), db ([groups,] cout).
    one_product (None: LaunchPolicy.train_one_product): a split launch in the fp16 scheme multiplies the high planes only (EGR_W_F16X1)."""
    cin, cout = x.c, dy.c
    interleaved = gx is not None or gy is not None      # groups = channel slices of ONE batch (x, dy: group 0's slice; gx / gy: element strides)
    if interleaved and (gx is None or gy is None):
        raise RuntimeError("egorear_amd.conv2d_wgrad: gx and gy go together")
    if dy.n != x.n or (not interleaved and x.n % groups):
        raise RuntimeError("egorear_amd.conv2d_wgrad: image counts do not match / not divisible by groups")
    ng = x.n if interleaved else x.n // groups
    if ((x.h + 2 * pad - kh) // stride + 1, (x.w + 2 * pad - kw) // stride + 1) != (dy.h, dy.w):
        raise RuntimeError("egorear_amd.conv2d_wgrad: dy does not match the forward output geometry")
    d = ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout = ng, x.h, x.w, cin, cout
    d.kh, d.kw, d.stride, d.pad, d.ho, d.wo = kh, kw, stride, pad, dy.h, dy.w
    d.ldx, d.ldy, d.rmap = x.ld, dy.ld, NMap(1, 0, 0)
    d.xmap, d.ymap = NMap(ng, x.nstride, 0), NMap(ng, dy.nstride, 0)
    K = kh * kw * cin
    d.groups, d.gx, d.gy, d.gw, d.gp = groups, (gx if interleaved else ng * x.nstride), (gy if interleaved else ng * dy.nstride), cout * K, cout
    if x6 is None and policy().wgrad_force and policy().wgrad_x6:
        x6 = "force"
    d.w_format = 3 if x6 == "force" else (1 if (policy().wgrad_x6 if x6 is None else x6) else 0)   # "force": the split kernel at any size
    # the fp16 scheme: split launches whose two operands carry abs-max records (made here with one read each when an arena is given)
    M = ng * dy.h * dy.w
    split = d.w_format == 3 or (d.w_format == 1 and M >= 1024 and 2.0 * M * cout * K * groups >= 4e9)
    if split:
        wgrad_records(x, dy, amax_arena)
    h2 = split and policy().h2 and x.amax is not None and dy.amax is not None
    h1 = h2 and (policy().train_one_product if one_product is None else bool(one_product))
    if h2:
        d.w_format |= W_F16X2 | (W_F16X1 if h1 else 0)
    shape_w, shape_b = ((groups, cout, K), (groups, cout)) if groups > 1 else ((cout, K), (cout,))
    if dw is None:
        dw = torch.empty(shape_w, device=x.t.device, dtype=torch.float32)
    elif dw.numel() != groups * cout * K:
        raise RuntimeError("egorear_amd.conv2d_wgrad: dw has the wrong size")
    if want_bias and db is None:
        db = torch.empty(shape_b, device=x.t.device, dtype=torch.float32)
    _launch("egr_conv2d_wgrad_f32", lib.egr_conv2d_wgrad_ex_f32, C.byref(d), _p(x.t), _p(dy.t), _p(_cont(dw, "dw")), _p(db),
            _p(workspace), workspace.numel(), 1 if accumulate else 0, _p(x.amax, torch.int32) if h2 else None,
            _p(dy.amax, torch.int32) if h2 else None, _stream(), flops=2.0 * dy.n * dy.h * dy.w * cout * K,
            tag=f"{('h1 ' if h1 else 'h2 ') if h2 else ''}G{groups} M{ng * dy.h * dy.w} N{cout} K{K} k{kh}s{stride} cin{cin}" if PROFILE is not None else "")
    return dw, db


def stem(img: torch.Tensor, view0: int, nviews: int, wpack, scale, shift, groups: int = 1) -> Img:
    """img (B, V, 3, H, W) NCHW contiguous.  Group g handles views [view0 + g*nviews, view0 + (g+1)*nviews) with its own
    weights (wpack (groups,64,148), scale/shift (groups,64)); output NHWC (groups*nviews*B, H/2, W/2, 64), view-major."""
    B, V, Cc, H, W = img.shape
    if Cc != 3:
        raise RuntimeError("egorear_amd.stem: 3-channel input expected")
    _cont(img, "input image batch")
    raw = scale is None and shift is None          # training mode: bare convolution
    if view0 + groups * nviews > V or wpack.numel() != groups * 64 * 148 or (not raw and (scale.numel() != groups * 64 or shift.numel() != groups * 64)):
        raise RuntimeError("egorear_amd.stem: views / weights mismatch")
    n = nviews * B
    y = torch.empty((groups * n, H // 2, W // 2, 64), device=img.device, dtype=torch.float32)
    base = img.reshape(-1)[view0 * 3 * H * W:]
    xmap = NMap(B, V * 3 * H * W, 3 * H * W)  # n = v*B + b -> (b*V + v) image
    _launch("egr_stem_conv7x7_f32", lib.egr_stem_conv7x7_f32, _p(base), xmap, n, H, W, _p(_cont(wpack, "stem weight")), _p(scale),
            _p(shift), _p(y), groups, nviews * 3 * H * W, _stream(),
            flops=2.0 * groups * n * (H // 2) * (W // 2) * 64 * 147, nbytes=4.0 * groups * n * (3 * H * W + (H // 2) * (W // 2) * 64))
    return Img(y)


def stem_pool(img: torch.Tensor, view0: int, nviews: int, wpack, scale, shift, groups: int = 1) -> Img:
    """stem() + maxpool(3, 2, 1) in one pass (eval mode): output NHWC (groups*nviews*B, H/4, W/4, 64)."""
    B, V, Cc, H, W = img.shape
    if Cc != 3:
        raise RuntimeError("egorear_amd.stem_pool: 3-channel input expected")
    _cont(img, "input image batch")
    if scale is None or shift is None:
        raise RuntimeError("egorear_amd.stem_pool: eval-mode BatchNorm scale / shift required")
    if view0 + groups * nviews > V or wpack.numel() != groups * 64 * 148 or scale.numel() != groups * 64 or shift.numel() != groups * 64:
        raise RuntimeError("egorear_amd.stem_pool: views / weights mismatch")
    n = nviews * B
    y = torch.empty((groups * n, H // 4, W // 4, 64), device=img.device, dtype=torch.float32)
    base = img.reshape(-1)[view0 * 3 * H * W:]
    xmap = NMap(B, V * 3 * H * W, 3 * H * W)
    _launch("egr_stem_conv7x7_pool_f32", lib.egr_stem_conv7x7_pool_f32, _p(base), xmap, n, H, W, _p(_cont(wpack, "stem weight")),
            _p(scale), _p(shift), _p(y), groups, nviews * 3 * H * W, _stream(),
            flops=2.0 * groups * n * (H // 2) * (W // 2) * 64 * 147, nbytes=4.0 * groups * n * (3 * H * W + (H // 4) * (W // 4) * 64))
    return Img(y)


def pack_stem_w6(wpack: torch.Tensor) -> torch.Tensor:
    """(groups, 64, 148) fp32 stem filters -> the split-bf16 bank of stem_x6 ((groups, egr_stem_w6_bytes()) uint8)."""
    if wpack.dim() != 3 or wpack.shape[1:] != (64, 148) or wpack.dtype != torch.float32:
        raise RuntimeError("egorear_amd.pack_stem_w6: (groups, 64, 148) fp32 expected")
    img = torch.empty((wpack.shape[0], int(lib.egr_stem_w6_bytes())), device=wpack.device, dtype=torch.uint8)
    _launch("egr_pack_stem_w6_f32", lib.egr_pack_stem_w6_f32, _p(_cont(wpack, "stem weight")), wpack.shape[0], _p(img, torch.uint8), _stream())
    return img


def pack_wstream(w: torch.Tensor):
    """(n, k) fp32 weights of a few-rows Linear -> (the weight-stream image (4 n k bytes) uint8, descale (n,)) (egr_pack_wstream_f32)."""
    if w.dim() != 2 or w.dtype != torch.float32 or w.shape[0] % 64 or w.shape[1] % 256:
        raise RuntimeError("egorear_amd.pack_wstream: (n % 64 == 0, k % 256 == 0) fp32 expected")
    n, k = w.shape
    img = torch.empty((int(lib.egr_wstream_image_bytes(n, k)),), device=w.device, dtype=torch.uint8)
    ds = torch.empty((n,), device=w.device, dtype=torch.float32)
    _launch("egr_pack_wstream_f32", lib.egr_pack_wstream_f32, _p(_cont(w, "weight")), n, k, _p(img, torch.uint8), _p(ds), _stream())
    return img, ds


def linear_wstream(x: torch.Tensor, img: torch.Tensor, descale: torch.Tensor, bias: Optional[torch.Tensor], act: int, workspace: torch.Tensor,
                   amax_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(x w^T + bias) for x (rows, k) with its abs-max record (x._egr_amax), w as pack_wstream's image: the weight-stream
    launch (egr_linear_wstream_f32).  More than 64 rows run as chunks of 64 (the weights are streamed once per chunk)."""
    rec = getattr(x, "_egr_amax", None)
    if rec is None:
        raise RuntimeError("egorear_amd.linear_wstream: the rows carry no abs-max record")
    n = descale.numel()
    rows, k = x.shape
    if x.dtype != torch.float32 or x.stride(1) != 1 or img.numel() != 4 * n * k:
        raise RuntimeError("egorear_amd.linear_wstream: operands do not match")
    y = torch.empty((rows, n), device=x.device, dtype=torch.float32)
    for r0 in range(0, rows, 64):
        r = min(64, rows - r0)
        need = int(lib.egr_linear_wstream_workspace_bytes(r, n, k))
        if need < 0 or workspace.numel() * workspace.element_size() < need:
            raise RuntimeError(f"egorear_amd.linear_wstream: workspace of {need} bytes needed")
        xr, yr = x[r0:r0 + r], y[r0:r0 + r]
        _launch("egr_linear_wstream_f32", lib.egr_linear_wstream_f32, _p(xr), xr.stride(0), r, k, _p(img, torch.uint8), _p(descale),
                _p(bias), n, act, _p(rec, torch.int32), _p(yr), yr.stride(0), _p(amax_out, torch.int32), _p(workspace, workspace.dtype),
                workspace.numel() * workspace.element_size(), _stream(), flops=2.0 * r * n * k, nbytes=4.0 * n * k + 4.0 * r * (n + k),
                tag="h2 wstream")
    if amax_out is not None:
        y._egr_amax = amax_out
    return y


def pack_stem_wh2(wpack: torch.Tensor):
    """(groups, 64, 148) fp32 stem filters -> (the fp16-scheme bank (groups, egr_stem_wh2_bytes()) uint8, its descale (groups, 64))."""
    if wpack.dim() != 3 or wpack.shape[1:] != (64, 148) or wpack.dtype != torch.float32:
        raise RuntimeError("egorear_amd.pack_stem_wh2: (groups, 64, 148) fp32 expected")
    img = torch.empty((wpack.shape[0], int(lib.egr_stem_wh2_bytes())), device=wpack.device, dtype=torch.uint8)
    ds = torch.empty((wpack.shape[0], 64), device=wpack.device, dtype=torch.float32)
    _launch("egr_pack_stem_wh2_f32", lib.egr_pack_stem_wh2_f32, _p(_cont(wpack, "stem weight")), wpack.shape[0], _p(img, torch.uint8), _p(ds), _stream())
    return img, ds


def stem_x6(img: torch.Tensor, view0: int, nviews: int, w6: torch.Tensor, scale, shift, groups: int = 1, pool: bool = False,
            amax_out: Optional[torch.Tensor] = None, w_descale: Optional[torch.Tensor] = None) -> Img:
    """stem() on the bf16 matrix cores (w6 from pack_stem_w6); pool=True: + maxpool(3, 2, 1) in the same pass (eval mode),
    output (groups*nviews*B, H/4, W/4, 64); amax_out (pool=True): the output's abs-max record (64 zeroed int32 slots)."""
    B, V, Cc, H, W = img.shape
    if Cc != 3:
        raise RuntimeError("egorear_amd.stem_x6: 3-channel input expected")
    _cont(img, "input image batch")
    raw = scale is None and shift is None
    if pool and raw:
        raise RuntimeError("egorear_amd.stem_x6: the fused max-pool needs the eval-mode BatchNorm scale / shift")
    h2 = w_descale is not None      # w6 is then the fp16-scheme bank of pack_stem_wh2
    if (view0 + groups * nviews > V or w6.dtype != torch.uint8
            or w6.numel() != groups * int(lib.egr_stem_wh2_bytes() if h2 else lib.egr_stem_w6_bytes())
            or (h2 and w_descale.numel() != groups * 64)
            or (not raw and (scale.numel() != groups * 64 or shift.numel() != groups * 64))):
        raise RuntimeError("egorear_amd.stem_x6: views / weights mismatch")
    n = nviews * B
    d = 4 if pool else 2
    y = torch.empty((groups * n, H // d, W // d, 64), device=img.device, dtype=torch.float32)
    base = img.reshape(-1)[view0 * 3 * H * W:]
    xmap = NMap(B, V * 3 * H * W, 3 * H * W)
    if amax_out is not None and (not pool or amax_out.numel() != 64 or amax_out.dtype != torch.int32):
        raise RuntimeError("egorear_amd.stem_x6: the abs-max record (64 int32 slots) goes with pool=True")
    if h2:
        _launch("egr_stem_conv7x7_x6_f32", lib.egr_stem_conv7x7_h2_f32, _p(base), xmap, n, H, W, _p(_cont(w6, "stem weight"), torch.uint8),
                _p(_cont(w_descale, "stem descale")), _p(scale), _p(shift), _p(y), 1 if pool else 0, groups, nviews * 3 * H * W,
                _p(amax_out, torch.int32), _stream(),
                flops=2.0 * groups * n * (H // 2) * (W // 2) * 64 * 147, nbytes=4.0 * groups * n * (3 * H * W + (H // d) * (W // d) * 64),
                tag="h2 pool" if pool else "h2")
    else:
        _launch("egr_stem_conv7x7_x6_f32", lib.egr_stem_conv7x7_x6_ex_f32, _p(base), xmap, n, H, W, _p(_cont(w6, "stem weight"), torch.uint8), _p(scale),
                _p(shift), _p(y), 1 if pool else 0, groups, nviews * 3 * H * W, _p(amax_out, torch.int32), _stream(),
                flops=2.0 * groups * n * (H // 2) * (W // 2) * 64 * 147, nbytes=4.0 * groups * n * (3 * H * W + (H // d) * (W // d) * 64),
                tag="x6 pool" if pool else "x6")
    out = Img(y)
    out.tag(amax_out)
    return out


def maxpool(x: Img, k: int, stride: int, pad: int) -> Img:
    if not x.t.is_contiguous():
        raise RuntimeError("egorear_amd.maxpool: contiguous NHWC input expected")
    ho = (x.h + 2 * pad - k) // stride + 1
    wo = (x.w + 2 * pad - k) // stride + 1
    y = torch.empty((x.n, ho, wo, x.c), device=x.t.device, dtype=torch.float32)
    _launch("egr_maxpool_nhwc_f32", lib.egr_maxpool_nhwc_f32, _p(x.t), _p(y), x.n, x.h, x.w, x.c, k, stride, pad, _stream(),
            nbytes=4.0 * x.n * x.c * (x.h * x.w + ho * wo))
    out = Img(y)
    out.tag(x.amax)     # max |max-pool(x)| <= max |x|: the input's record bounds the output
    return out


def upsample2x(x: Img, out: Optional[Img] = None, relu: bool = False) -> Img:
    if x.n > 1 and x.nstride != x.h * x.w * x.ld:
        raise RuntimeError("egorear_amd.upsample2x: images must be densely stacked")
    if out is None:
        out = Img(torch.empty((x.n, 2 * x.h, 2 * x.w, x.c), device=x.t.device, dtype=torch.float32))
    if (out.n, out.h, out.w, out.c) != (x.n, 2 * x.h, 2 * x.w, x.c) or (out.n > 1 and out.nstride != out.h * out.w * out.ld):
        raise RuntimeError("egorear_amd.upsample2x: bad output view")
    _launch("egr_upsample2x_nhwc_f32", lib.egr_upsample2x_nhwc_f32, _p(x.t), x.ld, _p(out.t), out.ld, x.n, x.h, x.w, x.c, 1 if relu else 0, _stream(),
            nbytes=4.0 * 5 * x.n * x.h * x.w * x.c)
    out.tag(x.amax)     # bilinear interpolation (+ ReLU) is a convex combination: the input's record bounds the output
    return out


def up2_relu_head(lo: Img, wgt: torch.Tensor, bias: Optional[torch.Tensor], planes: torch.Tensor, ymap: NMap, gy: int, groups: int = 1):
    """Upsample x2 + ReLU + final 1x1 conv of a heat-map head, straight into channel-major planes (see egorear_hip.h).
    lo: dense (groups*n, h, w, cin); wgt (groups, cout, cin) contiguous; image i of group g lands at planes.flat[g*gy + ymap(i)]."""
    if not lo.t.is_contiguous() or lo.n % groups:
        raise RuntimeError("egorear_amd.up2_relu_head: dense NHWC input with groups | n expected")
    cout, cin = wgt.shape[-2], wgt.shape[-1]
    npg = lo.n // groups
    if cin != lo.c or wgt.numel() != groups * cout * cin or (bias is not None and bias.numel() != groups * cout):
        raise RuntimeError("egorear_amd.up2_relu_head: weight / bias shape")
    ho, wo = 2 * lo.h, 2 * lo.w
    last = (groups - 1) * gy + (npg - 1) // ymap.n_inner * ymap.stride_outer + min(npg - 1, ymap.n_inner - 1) * ymap.stride_inner + cout * ho * wo
    if not planes.is_contiguous() or last > planes.numel():
        raise RuntimeError("egorear_amd.up2_relu_head: output map runs outside the tensor")
    _launch("egr_up2_relu_head_f32", lib.egr_up2_relu_head_f32, _p(lo.t), lo.n, lo.h, lo.w, cin, _p(_cont(wgt, "weight")), _p(bias), cout,
            _p(planes), ymap.n_inner, ymap.stride_inner, ymap.stride_outer, groups, gy, _stream(),
            flops=2.0 * lo.n * ho * wo * cout * cin, nbytes=4.0 * lo.n * (lo.h * lo.w * cin + cout * ho * wo))


def avgpool(x: Img) -> torch.Tensor:
    if not x.t.is_contiguous():
        raise RuntimeError("egorear_amd.avgpool: contiguous input expected")
    y = torch.empty((x.n, x.c), device=x.t.device, dtype=torch.float32)
    _launch("egr_avgpool_nhwc_f32", lib.egr_avgpool_nhwc_f32, _p(x.t), _p(y), x.n, x.h * x.w, x.c, _stream(),
            nbytes=4.0 * x.n * x.c * (x.h * x.w + 1))
    return y


def argmax_rows(hm: torch.Tensor, thr: float):
    """hm (..., H, W) contiguous -> anchors (rows,2) f32, maxvals (rows,), valid (rows,) u8, index (rows,) i32."""
    _cont(hm, "heatmap")
    H, W = hm.shape[-2:]
    rows = hm.numel() // (H * W)
    dev = hm.device
    anchors = torch.empty((rows, 2), device=dev, dtype=torch.float32)
    maxvals = torch.empty((rows,), device=dev, dtype=torch.float32)
    valid = torch.empty((rows,), device=dev, dtype=torch.uint8)
    index = torch.empty((rows,), device=dev, dtype=torch.int32)
    _launch("egr_argmax_rows_f32", lib.egr_argmax_rows_f32, _p(hm), rows, H, W, float(thr), _p(anchors), _p(maxvals), _p(valid, torch.uint8),
                                   _p(index, torch.int32), _stream(), nbytes=4.0 * hm.numel() + 17.0 * rows)
    return anchors, maxvals, valid, index


def _maps(hm: torch.Tensor, what: str):
    """(rows, H, W) of a contiguous (..., H, W) tensor of heat maps."""
    if hm.dim() < 2:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (..., H, W), got {tuple(hm.shape)}")
    _cont(hm, "heatmap")
    H, W = hm.shape[-2:]
    if H * W == 0 or hm.numel() == 0:
        raise ValueError(f"egorear_amd.{what}: empty heat maps {tuple(hm.shape)}")
    return hm.numel() // (H * W), H, W


def soft_argmax(hm: torch.Tensor, beta: float = 1.0, mode: int = 0, normalize: bool = False, thr: float = 0.0, want_probs: bool = False):
    """hm (..., H, W) contiguous -> coords (rows,2) f32 (x, y), maxvals (rows,), index (rows,) i32, valid (rows,) u8, stat (rows,2) f32,
    probs (rows,H,W) | None: egr_soft_argmax_f32, one read of the maps for the soft and the hard decode (mode 0 softmax, 1 relu mass)."""
    rows, H, W = _maps(hm, "soft_argmax")
    dev = hm.device
    coords = torch.empty((rows, 2), device=dev, dtype=torch.float32)
    maxvals = torch.empty((rows,), device=dev, dtype=torch.float32)
    index = torch.empty((rows,), device=dev, dtype=torch.int32)
    valid = torch.empty((rows,), device=dev, dtype=torch.uint8)
    stat = torch.empty((rows, 2), device=dev, dtype=torch.float32)
    probs = torch.empty((rows, H, W), device=dev, dtype=torch.float32) if want_probs else None
    _launch("egr_soft_argmax_f32", lib.egr_soft_argmax_f32, _p(hm), rows, H, W, float(beta), int(mode), 1 if normalize else 0, float(thr),
            _p(coords), _p(maxvals), _p(index, torch.int32), _p(valid, torch.uint8), _p(stat), _p(probs), _stream(),
            nbytes=4.0 * hm.numel() * (2 if want_probs else 1) + 25.0 * rows)
    return coords, maxvals, index, valid, stat, probs


def soft_argmax_bwd(hm: torch.Tensor, stat: torch.Tensor, coords: torch.Tensor, index: torch.Tensor, g_coords: torch.Tensor,
                    g_maxvals: Optional[torch.Tensor] = None, beta: float = 1.0, mode: int = 0, normalize: bool = False,
                    out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """Gradient of soft_argmax with respect to hm, from the forward's stat / coords / index: egr_soft_argmax_bwd_f32.  `out` (shaped like
    hm) is overwritten, or added to with accumulate=True; without `out` a new tensor is returned."""
    rows, H, W = _maps(hm, "soft_argmax_bwd")
    for t, n, what in ((stat, 2 * rows, "stat"), (coords, 2 * rows, "coords"), (index, rows, "index"), (g_coords, 2 * rows, "g_coords"),
                       (g_maxvals, rows, "g_maxvals")):
        if t is not None and (t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"egorear_amd.soft_argmax_bwd: {what} must be contiguous with {n} elements, got {tuple(t.shape)}")
    if out is None:
        if accumulate:
            raise ValueError("egorear_amd.soft_argmax_bwd: accumulate needs `out`")
        out = torch.empty_like(hm)
    elif out.shape != hm.shape or not out.is_contiguous():
        raise ValueError("egorear_amd.soft_argmax_bwd: `out` must be contiguous and shaped like the heat maps")
    _launch("egr_soft_argmax_bwd_f32", lib.egr_soft_argmax_bwd_f32, _p(hm), _p(stat), _p(coords), _p(index, torch.int32), _p(g_coords),
            _p(g_maxvals), rows, H, W, float(beta), int(mode), 1 if normalize else 0, 1 if accumulate else 0, _p(out), _stream(),
            nbytes=4.0 * hm.numel() * (3 if accumulate else 2) + 36.0 * rows)
    return out


def coord_l1(coords: torch.Tensor, index: torch.Tensor, valid: torch.Tensor, wid: int, weight: float, loss: torch.Tensor,
             want_grad: bool = True) -> Optional[torch.Tensor]:
    """loss (one device float64, overwritten) = weight * mean over valid maps of |x^ - x*| + |y^ - y*| with (x*, y*) = (index % wid,
    index // wid); returns g_coords (rows,2) = weight * sign / N_valid (zero where invalid) | None: egr_coord_l1_f32."""
    if loss.dtype != torch.float64 or loss.numel() != 1:
        raise ValueError("egorear_amd.coord_l1: loss must be one float64")
    rows = index.numel()
    if rows == 0 or coords.numel() != 2 * rows or valid.numel() != rows or not (coords.is_contiguous() and index.is_contiguous() and valid.is_contiguous()):
        raise ValueError("egorear_amd.coord_l1: coords (rows,2), index (rows,) and valid (rows,) must be contiguous and agree")
    g = torch.empty((rows, 2), device=coords.device, dtype=torch.float32) if want_grad else None
    _launch("egr_coord_l1_f32", lib.egr_coord_l1_f32, _p(coords), _p(index, torch.int32), _p(valid, torch.uint8), rows, int(wid), float(weight),
            _p(loss, torch.float64), _p(g), _stream(), nbytes=(13.0 + (8.0 if want_grad else 0.0)) * rows)
    return g


RAY_REC = 30      # floats of one camera.packed_rays() record (its layout: csrc/egr_rays.h)


# what the validators of the launches on ray records share; `named` are (tensor | None, name) pairs

def _on_device(what: str, *tensors, exc=RuntimeError):
    """There is no CPU path.  (Meta tensors pass: the fake implementations and a trace validate with them.)"""
    for t in tensors:
        if t is not None and not t.is_cuda and t.device.type != "meta":
            raise exc(f"egorear_amd.{what}: no CPU path - tensors must live on the HIP device")


def _rig(what: str, cams, ctm, B: int, V: int):
    if not 2 <= V <= 4:
        raise ValueError(f"egorear_amd.{what}: 2 to 4 views are supported, got {V}")
    if tuple(cams.shape) != (V, RAY_REC):
        raise ValueError(f"egorear_amd.{what}: cams must be {(V, RAY_REC)} (camera.packed_rays()), got {tuple(cams.shape)}")
    if ctm is not None and tuple(ctm.shape) != (B, V, 4, 4):
        raise ValueError(f"egorear_amd.{what}: coord_trans_mat must be {(B, V, 4, 4)}, got {tuple(ctm.shape)}")


def _float32(what: str, *named):
    for t, name in named:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"egorear_amd.{what}: float32 {name} expected, got {t.dtype}")


def _cotangents(what: str, *specs):
    for t, shape, name in specs:
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32):
            raise ValueError(f"egorear_amd.{what}: {name} must be a float32 {shape}, got {t.dtype} {tuple(t.shape)}")


def _contiguous(what: str, dense: bool, *named):
    # (dense: a launch reads its operands as they lie; the operators validate first and make them contiguous after)
    for t, name in named:
        if dense and t is not None and not t.is_contiguous():
            raise ValueError(f"egorear_amd.{what}: {name} must be contiguous")


def _positive(what: str, name: str, *values):
    if not all(v > 0.0 and math.isfinite(v) for v in values):
        raise ValueError(f"egorear_amd.{what}: {name} must be positive and finite, got {values!r}")


def _non_negative(what: str, name: str, value):
    if not (value >= 0.0 and math.isfinite(value)):
        raise ValueError(f"egorear_amd.{what}: {name} must be a non-negative finite number, got {value!r}")


def _tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, what: str, g_pts=None, g_cost=None, dense: bool = True):
    """(B, V, J) of a triangulation launch; every shape / dtype / parameter error as ValueError."""
    if coords.dim() != 4 or coords.shape[-1] != 2:
        raise ValueError(f"egorear_amd.{what}: coords must be (B, V, J, 2), got {tuple(coords.shape)}")
    B, V, J = (int(v) for v in coords.shape[:3])
    if B < 1 or J < 1:
        raise ValueError(f"egorear_amd.{what}: empty coords {tuple(coords.shape)}")
    if tuple(conf.shape) != (B, V, J):
        raise ValueError(f"egorear_amd.{what}: conf must be {(B, V, J)}, got {tuple(conf.shape)}")
    _rig(what, cams, ctm, B, V)
    _float32(what, (coords, "coords"), (conf, "conf"), (cams, "cams"), (ctm, "coord_trans_mat"))
    _positive(what, "the coordinate scales", sx, sy)
    _non_negative(what, "min_det_ratio", min_det_ratio)
    _cotangents(what, (g_pts, (B, J, 3), "g_pts"), (g_cost, (B, J), "g_cost"))
    _contiguous(what, dense, (coords, "coords"), (conf, "conf"), (cams, "cams"), (ctm, "coord_trans_mat"), (g_pts, "g_pts"), (g_cost, "g_cost"))
    return B, V, J


def triangulate(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor] = None, sx: float = 1.0,
                sy: float = 1.0, threshold: float = 0.5, min_det_ratio: float = 1e-6):
    """coords (B,V,J,2), conf (B,V,J), cams (V,30) = camera.packed_rays(), ctm (B,V,4,4) | None (the syn rig) -> pts (B,J,3) cm,
    cost (B,J) cm^2, resid (B,V,J) cm, ok (B,J) u8: egr_triangulate_f32, the least-squares intersection of the views' fisheye rays."""
    B, V, J = _tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, "triangulate")
    _on_device("triangulate", coords, conf, cams, ctm)
    dev = coords.device
    pts = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
    cost = torch.empty((B, J), device=dev, dtype=torch.float32)
    resid = torch.empty((B, V, J), device=dev, dtype=torch.float32)
    ok = torch.empty((B, J), device=dev, dtype=torch.uint8)
    _launch("egr_triangulate_f32", lib.egr_triangulate_f32, _p(coords), _p(conf), _p(cams), _p(ctm), B, V, J, float(sx), float(sy),
            float(threshold), float(min_det_ratio), _p(pts), _p(cost), _p(resid), _p(ok, torch.uint8), _stream(),
            nbytes=B * J * (V * (16.0 + (64.0 if ctm is not None else 0.0)) + 17.0))
    return pts, cost, resid, ok


def triangulate_bwd(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], g_pts: Optional[torch.Tensor],
                    g_cost: Optional[torch.Tensor], sx: float = 1.0, sy: float = 1.0, threshold: float = 0.5, min_det_ratio: float = 1e-6):
    """Gradients of triangulate's pts and cost with respect to coords and conf, (B,V,J,2) and (B,V,J): egr_triangulate_bwd_f32 (the
    forward is recomputed from the operands).  g_pts (B,J,3) and g_cost (B,J) may each be None for zeros."""
    B, V, J = _tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, "triangulate_bwd", g_pts, g_cost)
    _on_device("triangulate_bwd", coords, conf, cams, ctm, g_pts, g_cost)
    dev = coords.device
    g_coords = torch.empty((B, V, J, 2), device=dev, dtype=torch.float32)
    g_conf = torch.empty((B, V, J), device=dev, dtype=torch.float32)
    _launch("egr_triangulate_bwd_f32", lib.egr_triangulate_bwd_f32, _p(coords), _p(conf), _p(cams), _p(ctm), B, V, J, float(sx), float(sy),
            float(threshold), float(min_det_ratio), _p(g_pts), _p(g_cost), _p(g_coords), _p(g_conf), _stream(),
            nbytes=B * J * (V * (28.0 + (64.0 if ctm is not None else 0.0)) + 16.0))
    return g_coords, g_conf


VOLUME_MAX_ELEMS = 16384      # V * H * W floats of one LDS image of egr_volume.hip: four 64 x 64 maps
VOLUME_MIN_GRID, VOLUME_MAX_GRID = 2, 32


def _volume_operands(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, what: str, g_pose=None, g_peak=None, dense: bool = True):
    """(B, V, J, H, W) of a volumetric-fusion launch; every shape / dtype / parameter error as ValueError (dense: the operands must
    be contiguous too - a launch reads them as they lie)."""
    if hm.dim() != 5:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (B, V, J, H, W), got {tuple(hm.shape)}")
    B, V, J, H, W = (int(v) for v in hm.shape)
    if B < 1 or J < 1 or H < 1 or W < 1:
        raise ValueError(f"egorear_amd.{what}: empty heat maps {tuple(hm.shape)}")
    _rig(what, cams, ctm, B, V)
    if V * H * W > VOLUME_MAX_ELEMS:
        raise ValueError(f"egorear_amd.{what}: the V * H * W = {V * H * W} elements of a joint's maps exceed the {VOLUME_MAX_ELEMS} the "
                         f"kernel holds in LDS")
    if isinstance(grid, bool) or not isinstance(grid, int) or not VOLUME_MIN_GRID <= grid <= VOLUME_MAX_GRID:
        raise ValueError(f"egorear_amd.{what}: grid must be an integer in {VOLUME_MIN_GRID}..{VOLUME_MAX_GRID}, got {grid!r}")
    _positive(what, "the cube's side (cm)", cube)
    _positive(what, "beta", beta)
    if tuple(conf.shape) != (B, V, J):
        raise ValueError(f"egorear_amd.{what}: conf must be {(B, V, J)}, got {tuple(conf.shape)}")
    if tuple(centers.shape) != (B, J, 3):
        raise ValueError(f"egorear_amd.{what}: centers must be {(B, J, 3)}, got {tuple(centers.shape)}")
    if center_ok is not None and (tuple(center_ok.shape) != (B, J) or center_ok.dtype != torch.uint8):
        raise ValueError(f"egorear_amd.{what}: center_ok must be a uint8 {(B, J)}, got {center_ok.dtype} {tuple(center_ok.shape)}")
    floats = ((hm, "heat maps"), (conf, "conf"), (centers, "centers"), (cams, "cams"), (ctm, "coord_trans_mat"))
    _float32(what, *floats)
    _cotangents(what, (g_pose, (B, J, 3), "g_pose"), (g_peak, (B, J), "g_peak"))
    _contiguous(what, dense, *floats, (center_ok, "center_ok"), (g_pose, "g_pose"), (g_peak, "g_peak"))
    return B, V, J, H, W


def volume_fuse(hm: torch.Tensor, conf: torch.Tensor, centers: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor] = None,
                center_ok: Optional[torch.Tensor] = None, grid: int = 16, cube: float = 40.0, beta: float = 100.0, threshold: float = 0.5):
    """hm (B,V,J,H,W), conf (B,V,J), centers (B,J,3) cm, cams (V,30) = camera.packed_rays(), ctm (B,V,4,4) | None (the syn rig),
    center_ok (B,J) u8 | None -> pose (B,J,3) cm, peak (B,J), index (B,J) i32, spread (B,J) cm, ok (B,J) u8: egr_volume_fuse_f32, the
    3-D soft-argmax of the views' heat maps sampled at the projections of a grid^3 voxel cube of side `cube` around each centre."""
    B, V, J, H, W = _volume_operands(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, "volume_fuse")
    _on_device("volume_fuse", hm, conf, centers, cams, ctm, center_ok)
    dev = hm.device
    pose = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
    peak = torch.empty((B, J), device=dev, dtype=torch.float32)
    index = torch.empty((B, J), device=dev, dtype=torch.int32)
    spread = torch.empty((B, J), device=dev, dtype=torch.float32)
    ok = torch.empty((B, J), device=dev, dtype=torch.uint8)
    _launch("egr_volume_fuse_f32", lib.egr_volume_fuse_f32, _p(hm), _p(conf), _p(centers), _p(cams), _p(ctm), _p(center_ok, torch.uint8),
            B, V, J, H, W, int(grid), float(cube), float(beta), float(threshold), _p(pose), _p(peak), _p(index, torch.int32), _p(spread),
            _p(ok, torch.uint8), _stream(), nbytes=4.0 * B * V * J * H * W + B * J * (V * 4.0 + 38.0))
    return pose, peak, index, spread, ok


def volume_fuse_bwd(hm: torch.Tensor, conf: torch.Tensor, centers: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor],
                    center_ok: Optional[torch.Tensor], g_pose: Optional[torch.Tensor], g_peak: Optional[torch.Tensor], grid: int = 16,
                    cube: float = 40.0, beta: float = 100.0, threshold: float = 0.5) -> torch.Tensor:
    """Gradient of volume_fuse's pose and peak with respect to hm, (B,V,J,H,W): egr_volume_fuse_bwd_f32 (the forward is recomputed
    from the operands; every element is written).  g_pose (B,J,3) and g_peak (B,J) may each be None for zeros."""
    B, V, J, H, W = _volume_operands(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, "volume_fuse_bwd", g_pose, g_peak)
    _on_device("volume_fuse_bwd", hm, conf, centers, cams, ctm, center_ok, g_pose, g_peak)
    g_hm = torch.empty((B, V, J, H, W), device=hm.device, dtype=torch.float32)
    _launch("egr_volume_fuse_bwd_f32", lib.egr_volume_fuse_bwd_f32, _p(hm), _p(conf), _p(centers), _p(cams), _p(ctm),
            _p(center_ok, torch.uint8), B, V, J, H, W, int(grid), float(cube), float(beta), float(threshold), _p(g_pose), _p(g_peak),
            _p(g_hm), _stream(), nbytes=8.0 * B * V * J * H * W + B * J * (V * 4.0 + 28.0))
    return g_hm


PEAKS_MAX_ELEMS = 4096        # H * W floats of one LDS image of egr_peaks.hip
PEAKS_MAX_K, PEAKS_MAX_NMS, PEAKS_MAX_REFINE = 4, 3, 3


def _int_in(v, lo: int, hi: int) -> bool:
    return isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi


def _peaks_operands(hm, k, nms_radius, refine_radius, beta, min_score, what: str, dense: bool = True):
    """(lead shape, rows, H, W) of a peaks launch over (..., H, W) maps; every shape / dtype / parameter error as ValueError."""
    if hm.dim() < 2:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (..., H, W), got {tuple(hm.shape)}")
    if hm.dtype != torch.float32:
        raise ValueError(f"egorear_amd.{what}: float32 heat maps expected, got {hm.dtype}")
    H, W = int(hm.shape[-2]), int(hm.shape[-1])
    if hm.numel() == 0 or not 1 <= H * W <= PEAKS_MAX_ELEMS:
        raise ValueError(f"egorear_amd.{what}: maps must hold between 1 and {PEAKS_MAX_ELEMS} elements, got {tuple(hm.shape)}")
    if not _int_in(k, 1, PEAKS_MAX_K):
        raise ValueError(f"egorear_amd.{what}: k must be an integer in 1..{PEAKS_MAX_K}, got {k!r}")
    if not _int_in(nms_radius, 1, PEAKS_MAX_NMS):
        raise ValueError(f"egorear_amd.{what}: nms_radius must be an integer in 1..{PEAKS_MAX_NMS}, got {nms_radius!r}")
    if not _int_in(refine_radius, 0, PEAKS_MAX_REFINE):
        raise ValueError(f"egorear_amd.{what}: refine_radius must be an integer in 0..{PEAKS_MAX_REFINE}, got {refine_radius!r}")
    _positive(what, "beta", beta)
    if not math.isfinite(min_score):
        raise ValueError(f"egorear_amd.{what}: the score threshold must be finite, got {min_score!r}")
    _contiguous(what, dense, (hm, "heat maps"))
    return tuple(hm.shape[:-2]), hm.numel() // (H * W), H, W


def find_peaks(hm: torch.Tensor, k: int = 3, nms_radius: int = 1, refine_radius: int = 2, beta: float = 100.0, min_score: float = 0.5):
    """hm (..., H, W) contiguous, H * W <= 4096 -> coords (rows,k,2) f32 (x, y) heat-map pixels, score (rows,k), index (rows,k) i32,
    count (rows,) i32: egr_peaks_f32, the k best local maxima of every map (value, then smaller flat index), each refined over its
    (2 refine_radius + 1)^2 window.  Slots past count: coords 0, score 0, index -1."""
    _, rows, H, W = _peaks_operands(hm, k, nms_radius, refine_radius, beta, min_score, "find_peaks")
    _on_device("find_peaks", hm)
    dev = hm.device
    coords = torch.empty((rows, k, 2), device=dev, dtype=torch.float32)
    score = torch.empty((rows, k), device=dev, dtype=torch.float32)
    index = torch.empty((rows, k), device=dev, dtype=torch.int32)
    count = torch.empty((rows,), device=dev, dtype=torch.int32)
    _launch("egr_peaks_f32", lib.egr_peaks_f32, _p(hm), rows, H, W, int(k), int(nms_radius), int(refine_radius), float(beta), float(min_score),
            _p(coords), _p(score), _p(index, torch.int32), _p(count, torch.int32), _stream(), nbytes=4.0 * hm.numel() + rows * (16.0 * k + 4.0))
    return coords, score, index, count


def _consensus_operands(cand, cscore, cindex, cams, ctm, sx, sy, max_reproj, min_views, min_det_ratio, what: str, dense: bool = True):
    """(B, V, J, K) of a consensus launch; every shape / dtype / parameter error as ValueError."""
    if cand.dim() != 5 or cand.shape[-1] != 2:
        raise ValueError(f"egorear_amd.{what}: candidates must be (B, V, J, K, 2), got {tuple(cand.shape)}")
    B, V, J, K = (int(v) for v in cand.shape[:4])
    if not 1 <= K <= PEAKS_MAX_K:
        raise ValueError(f"egorear_amd.{what}: 1 to {PEAKS_MAX_K} candidates per view are supported, got {K}")
    if B < 1 or J < 1:
        raise ValueError(f"egorear_amd.{what}: empty candidates {tuple(cand.shape)}")
    if tuple(cscore.shape) != (B, V, J, K) or tuple(cindex.shape) != (B, V, J, K):
        raise ValueError(f"egorear_amd.{what}: scores and indices must be {(B, V, J, K)}, got {tuple(cscore.shape)} and {tuple(cindex.shape)}")
    _rig(what, cams, ctm, B, V)
    floats = ((cand, "candidates"), (cscore, "scores"), (cams, "cams"), (ctm, "coord_trans_mat"))
    _float32(what, *floats)
    if cindex.dtype != torch.int32:
        raise ValueError(f"egorear_amd.{what}: int32 indices expected, got {cindex.dtype}")
    _positive(what, "the coordinate scales", sx, sy)
    _positive(what, "max_reproj", max_reproj)
    if not _int_in(min_views, 2, V):
        raise ValueError(f"egorear_amd.{what}: min_views must be an integer in 2..{V}, got {min_views!r}")
    _non_negative(what, "min_det_ratio", min_det_ratio)
    _contiguous(what, dense, *floats, (cindex, "indices"))
    return B, V, J, K


def consensus(cand: torch.Tensor, cscore: torch.Tensor, cindex: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor] = None,
              sx: float = 1.0, sy: float = 1.0, max_reproj: float = 2.0, min_views: int = 2, min_det_ratio: float = 1e-6):
    """cand (B,V,J,K,2), cscore (B,V,J,K), cindex (B,V,J,K) i32 = find_peaks' outputs, cams (V,30), ctm (B,V,4,4) | None -> choice (B,V,J)
    i32, sel_coords (B,V,J,2), sel_conf (B,V,J), score (B,J), inliers (B,J) i32, hyp (B,J) i32: egr_consensus_f32, per joint the
    candidates the views agree on - the two-view hypothesis whose reprojections the views' candidates support best."""
    B, V, J, K = _consensus_operands(cand, cscore, cindex, cams, ctm, sx, sy, max_reproj, min_views, min_det_ratio, "consensus")
    _on_device("consensus", cand, cscore, cindex, cams, ctm)
    dev = cand.device
    choice = torch.empty((B, V, J), device=dev, dtype=torch.int32)
    sel_coords = torch.empty((B, V, J, 2), device=dev, dtype=torch.float32)
    sel_conf = torch.empty((B, V, J), device=dev, dtype=torch.float32)
    score = torch.empty((B, J), device=dev, dtype=torch.float32)
    inliers = torch.empty((B, J), device=dev, dtype=torch.int32)
    hyp = torch.empty((B, J), device=dev, dtype=torch.int32)
    _launch("egr_consensus_f32", lib.egr_consensus_f32, _p(cand), _p(cscore), _p(cindex, torch.int32), _p(cams), _p(ctm), B, V, J, K, float(sx),
            float(sy), float(max_reproj), int(min_views), float(min_det_ratio), _p(choice, torch.int32), _p(sel_coords), _p(sel_conf),
            _p(score), _p(inliers, torch.int32), _p(hyp, torch.int32), _stream(),
            nbytes=B * J * (V * (16.0 * K + 16.0 + (64.0 if ctm is not None else 0.0)) + 12.0))
    return choice, sel_coords, sel_conf, score, inliers, hyp


SKELETON_MAX_J = 16           # joints of one tree of egr_skeleton.hip: a lane a joint, 4 bits a parent
SKELETON_MAX_ITERATIONS = 256


def _parents(what: str, parents, J: int):
    """The parent table as a list of J integers (host memory: it travels to the kernel by value): parents[0] == 0 and
    0 <= parents[j] < j."""
    if isinstance(parents, torch.Tensor):
        if parents.device.type != "cpu" or parents.dtype.is_floating_point or parents.dim() != 1:
            raise ValueError(f"egorear_amd.{what}: parents must be a sequence of integers or a 1-D integer tensor in host memory")
        parents = parents.tolist()
    try:
        table = [int(v) for v in parents]
        exact = all(not isinstance(v, bool) and int(v) == v for v in parents)
    except (TypeError, ValueError):
        raise ValueError(f"egorear_amd.{what}: parents must be a sequence of integers, got {parents!r}") from None
    if not 1 <= J <= SKELETON_MAX_J:
        raise ValueError(f"egorear_amd.{what}: 1 to {SKELETON_MAX_J} joints are supported, got {J}")
    if not exact or len(table) != J:
        raise ValueError(f"egorear_amd.{what}: parents must be {J} integers, got {parents!r}")
    if table[0] != 0 or any(not 0 <= table[j] < j for j in range(1, J)):
        raise ValueError(f"egorear_amd.{what}: parents[0] must be 0 and 0 <= parents[j] < j (a parent comes before its children), got {table}")
    return table


def _host_table(table):
    return (C.c_int32 * len(table))(*table)


def _bone_length(what: str, bone_length, B: int, J: int) -> int:
    """1 when the lengths are per frame (B, J), 0 for one (J) table."""
    if tuple(bone_length.shape) not in ((J,), (B, J)):
        raise ValueError(f"egorear_amd.{what}: bone_length must be {(J,)} or {(B, J)}, got {tuple(bone_length.shape)}")
    return int(bone_length.dim() == 2)


def _flags(what: str, t, shape, name: str):
    if tuple(t.shape) != shape or t.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"egorear_amd.{what}: {name} must be a uint8 or bool {shape}, got {t.dtype} {tuple(t.shape)}")
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _fit_parameters(what: str, bone_weight, prior_weight, iterations):
    _non_negative(what, "bone_weight", bone_weight)
    _non_negative(what, "prior_weight", prior_weight)
    if not _int_in(iterations, 1, SKELETON_MAX_ITERATIONS):
        raise ValueError(f"egorear_amd.{what}: iterations must be an integer in 1..{SKELETON_MAX_ITERATIONS}, got {iterations!r}")


def _skeleton_parameters(B: int, J: int, parents, bone_length, init, init_ok, bone_weight, prior_weight, iterations, what: str,
                         dense: bool = True):
    """What a skeleton fit takes besides the triangulation's operands -> (the host parent table, per-frame lengths?).  `init` and
    `init_ok` may be None where a chain makes them itself (decode.decode_joints_3d_skeleton validates before its first launch)."""
    table = _parents(what, parents, J)
    per_frame = _bone_length(what, bone_length, B, J)
    if init is not None and tuple(init.shape) != (B, J, 3):
        raise ValueError(f"egorear_amd.{what}: init must be {(B, J, 3)}, got {tuple(init.shape)}")
    if init_ok is not None:
        _flags(what, init_ok, (B, J), "init_ok")
    _float32(what, (bone_length, "bone_length"), (init, "init"))
    _fit_parameters(what, bone_weight, prior_weight, iterations)
    _contiguous(what, dense, (bone_length, "bone_length"), (init, "init"), (init_ok, "init_ok"))
    return table, per_frame


def _skeleton_operands(coords, conf, cams, ctm, parents, bone_length, init, init_ok, sx, sy, min_det_ratio, bone_weight, prior_weight,
                       iterations, what: str, dense: bool = True):
    """(B, V, J, the host parent table, per-frame lengths?) of a skeleton fit; every shape / dtype / parameter error as ValueError."""
    B, V, J = _tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, what, dense=dense)
    if init is None or init_ok is None:
        raise ValueError(f"egorear_amd.{what}: init and init_ok are required")
    table, per_frame = _skeleton_parameters(B, J, parents, bone_length, init, init_ok, bone_weight, prior_weight, iterations, what, dense)
    return B, V, J, table, per_frame


def skeleton_fit(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], parents, bone_length: torch.Tensor,
                 init: torch.Tensor, init_ok: torch.Tensor, sx: float = 1.0, sy: float = 1.0, threshold: float = 0.5,
                 min_det_ratio: float = 1e-6, bone_weight: float = 1.0, prior_weight: float = 0.0, iterations: int = 16):
    """coords (B,V,J,2), conf (B,V,J), cams (V,30), ctm (B,V,4,4) | None as for triangulate; parents: J host integers; bone_length (J) |
    (B,J) cm; init (B,J,3) cm, init_ok (B,J) u8 -> pose (B,J,3), ray_cost (B,J), bone (B,J), valid (B,J) u8, energy0 (B), energy (B),
    grad (B), steps (B) i32: egr_skeleton_fit_f32, the joints that minimise the rays' distances plus bone_weight * the squared
    bone-length errors plus prior_weight * the squared distances from init (include/egorear_hip.h states the energy and the solver)."""
    B, V, J, table, per_frame = _skeleton_operands(coords, conf, cams, ctm, parents, bone_length, init, init_ok, sx, sy, min_det_ratio,
                                                   bone_weight, prior_weight, iterations, "skeleton_fit")
    _on_device("skeleton_fit", coords, conf, cams, ctm, bone_length, init, init_ok)
    init_ok = _flags("skeleton_fit", init_ok, (B, J), "init_ok")
    dev = coords.device
    pose = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
    ray_cost, bone = (torch.empty((B, J), device=dev, dtype=torch.float32) for _ in range(2))
    valid = torch.empty((B, J), device=dev, dtype=torch.uint8)
    energy0, energy, grad = (torch.empty((B,), device=dev, dtype=torch.float32) for _ in range(3))
    steps = torch.empty((B,), device=dev, dtype=torch.int32)
    _launch("egr_skeleton_fit_f32", lib.egr_skeleton_fit_f32, _p(coords), _p(conf), _p(cams), _p(ctm), _host_table(table), _p(bone_length),
            per_frame,
            _p(init), _p(init_ok, torch.uint8), B, V, J, float(sx), float(sy), float(threshold), float(min_det_ratio), float(bone_weight),
            float(prior_weight), int(iterations), _p(pose), _p(ray_cost), _p(bone), _p(valid, torch.uint8), _p(energy0), _p(energy), _p(grad),
            _p(steps, torch.int32), _stream(), nbytes=B * (J * (V * 12.0 + 38.0) + (V * 64.0 if ctm is not None else 0.0) + 16.0))
    return pose, ray_cost, bone, valid, energy0, energy, grad, steps


def _pose_operands(pose, valid, parents, what: str, dense: bool = True):
    """(B, J, the host parent table) of the launches on fitted poses; every shape / dtype error as ValueError."""
    if pose.dim() != 3 or pose.shape[-1] != 3:
        raise ValueError(f"egorear_amd.{what}: pose must be (B, J, 3), got {tuple(pose.shape)}")
    B, J = int(pose.shape[0]), int(pose.shape[1])
    if B < 1:
        raise ValueError(f"egorear_amd.{what}: empty pose {tuple(pose.shape)}")
    table = _parents(what, parents, J)
    _flags(what, valid, (B, J), "valid")
    _float32(what, (pose, "pose"))
    _contiguous(what, dense, (pose, "pose"), (valid, "valid"))
    return B, J, table


def bone_lengths(pose: torch.Tensor, valid: torch.Tensor, parents):
    """pose (B,J,3), valid (B,J) u8, parents: J host integers -> length (J), spread (J), count (J) i32: egr_bone_lengths_f32, mean and
    standard deviation of every bone over the frames of the clip in which both of its ends are valid."""
    B, J, table = _pose_operands(pose, valid, parents, "bone_lengths")
    _on_device("bone_lengths", pose, valid)
    valid = _flags("bone_lengths", valid, (B, J), "valid")
    dev = pose.device
    length, spread = (torch.empty((J,), device=dev, dtype=torch.float32) for _ in range(2))
    count = torch.empty((J,), device=dev, dtype=torch.int32)
    _launch("egr_bone_lengths_f32", lib.egr_bone_lengths_f32, _p(pose), _p(valid, torch.uint8), _host_table(table), B, J, _p(length), _p(spread),
            _p(count, torch.int32), _stream(), nbytes=B * J * 26.0 + J * 12.0)
    return length, spread, count


def _resize_operands(pose, valid, bone_length, parents, what: str, dense: bool = True):
    B, J, table = _pose_operands(pose, valid, parents, what, dense)
    per_frame = _bone_length(what, bone_length, B, J)
    _float32(what, (bone_length, "bone_length"))
    _contiguous(what, dense, (bone_length, "bone_length"))
    return B, J, table, per_frame


def skeleton_resize(pose: torch.Tensor, valid: torch.Tensor, bone_length: torch.Tensor, parents) -> torch.Tensor:
    """pose (B,J,3), valid (B,J) u8, bone_length (J) | (B,J) cm, parents: J host integers -> the pose with every bone between two valid
    joints set to its length along the kinematic chain: egr_skeleton_resize_f32, the reference's Skeleton._skeleton_resize in cm."""
    B, J, table, per_frame = _resize_operands(pose, valid, bone_length, parents, "skeleton_resize")
    _on_device("skeleton_resize", pose, valid, bone_length)
    valid = _flags("skeleton_resize", valid, (B, J), "valid")
    out = torch.empty_like(pose)
    _launch("egr_skeleton_resize_f32", lib.egr_skeleton_resize_f32, _p(pose), _p(valid, torch.uint8), _host_table(table), _p(bone_length), per_frame,
            B, J,
            _p(out), _stream(), nbytes=B * J * 29.0)
    return out


RIG_MAX_ITERATIONS = 256


def _rig_fixed(what: str, fixed, V: int):
    """The held cameras as a list of V flags (host memory: they travel to the kernel by value); None holds view 0 alone."""
    if fixed is None:
        return [v == 0 for v in range(V)]
    if isinstance(fixed, torch.Tensor):
        if fixed.dim() != 1 or fixed.dtype.is_floating_point or fixed.device.type == "meta":
            raise ValueError(f"egorear_amd.{what}: fixed must be a sequence of {V} flags or a ({V},) bool tensor with data")
        fixed = fixed.tolist()
    try:
        flags = [bool(f) for f in fixed]
        exact = all(isinstance(f, (bool, int)) and f in (0, 1) for f in fixed)
    except (TypeError, ValueError):
        raise ValueError(f"egorear_amd.{what}: fixed must be a sequence of {V} flags, got {fixed!r}") from None
    if not exact or len(flags) != V:
        raise ValueError(f"egorear_amd.{what}: fixed must be {V} flags, one a view, got {fixed!r}")
    return flags


def _rig_operands(coords, conf, cams, ctm, fixed, sx, sy, min_det_ratio, prior_weight, iterations, what: str, dense: bool = True):
    """(B, V, J, the held cameras, per-frame matrices?) of a rig refinement; every shape / dtype / parameter error as ValueError.
    coord_trans_mat may be (B, V, 4, 4) or (1, V, 4, 4), one rig for the clip."""
    if coords.dim() != 4 or coords.shape[-1] != 2:
        raise ValueError(f"egorear_amd.{what}: coords must be (B, V, J, 2), got {tuple(coords.shape)}")
    B, V = int(coords.shape[0]), int(coords.shape[1])
    per_frame = 1
    if ctm is not None and ctm.dim() == 4 and B > 1 and tuple(ctm.shape) == (1, V, 4, 4):
        per_frame = 0
    B, V, J = _tri_operands(coords, conf, cams, None if not per_frame else ctm, sx, sy, min_det_ratio, what, dense=dense)
    if not per_frame:
        _float32(what, (ctm, "coord_trans_mat"))
        _contiguous(what, dense, (ctm, "coord_trans_mat"))
    if B * J >= 1 << 28:
        raise ValueError(f"egorear_amd.{what}: B * J must stay below 2^28, got {tuple(coords.shape)}")
    flags = _rig_fixed(what, fixed, V)
    _non_negative(what, "prior_weight", prior_weight)
    if not _int_in(iterations, 1, RIG_MAX_ITERATIONS):
        raise ValueError(f"egorear_amd.{what}: iterations must be an integer in 1..{RIG_MAX_ITERATIONS}, got {iterations!r}")
    return B, V, J, flags, per_frame


def rig_refine(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor] = None, fixed=None, sx: float = 1.0,
               sy: float = 1.0, threshold: float = 0.5, min_det_ratio: float = 1e-6, prior_weight: float = 0.0, iterations: int = 8):
    """coords (B,V,J,2), conf (B,V,J), cams (V,30), ctm (B,V,4,4) | (1,V,4,4) | None as for triangulate; fixed: V host flags (None:
    view 0) -> rotation (V,3) rad, matrix (V,3,3), ctm_out (B,V,4,4), cost0 (1), cost (1), pairs (1) i32, steps (1) i32, grad (1),
    valid (1) u8: egr_rig_refine_f32, the rotations of the free cameras about their own centres that minimise the rays' distances over
    the clip (include/egorear_hip.h states the objective and the solver).  The fp64 workspace is allocated here, like the outputs."""
    B, V, J, flags, per_frame = _rig_operands(coords, conf, cams, ctm, fixed, sx, sy, min_det_ratio, prior_weight, iterations, "rig_refine")
    _on_device("rig_refine", coords, conf, cams, ctm)
    dev = coords.device
    nbytes_ws = int(lib.egr_rig_refine_workspace_bytes(B, V, J))
    ws = torch.empty((nbytes_ws // 8,), device=dev, dtype=torch.float64)
    rotation = torch.empty((V, 3), device=dev, dtype=torch.float32)
    matrix = torch.empty((V, 3, 3), device=dev, dtype=torch.float32)
    ctm_out = torch.empty((B, V, 4, 4), device=dev, dtype=torch.float32)
    cost0, cost, grad = (torch.empty((1,), device=dev, dtype=torch.float32) for _ in range(3))
    pairs, steps = (torch.empty((1,), device=dev, dtype=torch.int32) for _ in range(2))
    valid = torch.empty((1,), device=dev, dtype=torch.uint8)
    mask = sum(1 << v for v, f in enumerate(flags) if f)
    _launch("egr_rig_refine_f32", lib.egr_rig_refine_f32, _p(coords), _p(conf), _p(cams), _p(ctm), per_frame, B, V, J, float(sx), float(sy),
            float(threshold), float(min_det_ratio), mask, float(prior_weight), int(iterations), _p(ws, torch.float64), nbytes_ws, _p(rotation),
            _p(matrix), _p(ctm_out), _p(cost0), _p(cost), _p(pairs, torch.int32), _p(steps, torch.int32), _p(grad), _p(valid, torch.uint8),
            _stream(), nbytes=B * J * V * (12.0 + 32.0 * (iterations + 2)) + B * V * 64.0)
    return rotation, matrix, ctm_out, cost0, cost, pairs, steps, grad, valid


TRAJECTORY_MAX_T = 4096           # frames of one clip of egr_trajectory.hip
TRAJECTORY_MAX_REWEIGHTS = 16
TRAJECTORY_FWD_SLOTS, TRAJECTORY_BWD_SLOTS = 5, 8      # fp64 workspace planes of T * N * J: the two sub-diagonals and 3 / 6 right-hand sides


def _trajectory_parameters(what: str, vel_weight, accel_weight, huber, reweights, max_gap):
    """The penalty, Huber and gap conventions of the clip decoders (egr_trajectory.hip, egr_raytrack.hip)."""
    _non_negative(what, "vel_weight", vel_weight)
    _non_negative(what, "accel_weight", accel_weight)
    if not (vel_weight > 0.0 or accel_weight > 0.0):
        raise ValueError(f"egorear_amd.{what}: vel_weight and accel_weight must not both be zero")
    _non_negative(what, "huber", huber)
    if not _int_in(reweights, 0, TRAJECTORY_MAX_REWEIGHTS):
        raise ValueError(f"egorear_amd.{what}: reweights must be an integer in 0..{TRAJECTORY_MAX_REWEIGHTS}, got {reweights!r}")
    if (reweights > 0) != (huber > 0.0):
        raise ValueError(f"egorear_amd.{what}: huber > 0 and reweights > 0 go together (the plain form has both 0), got huber {huber!r}, "
                         f"reweights {reweights!r}")
    if not _int_in(max_gap, 0, (1 << 31) - 1):
        raise ValueError(f"egorear_amd.{what}: max_gap must be a non-negative integer, got {max_gap!r}")


def _trajectory_operands(pose, weight, obs, vel_weight, accel_weight, huber, reweights, max_gap, what: str, g_pose=None, dense: bool = True):
    """(N, T, J) of a trajectory launch; every shape / dtype / parameter error as ValueError."""
    if pose.dim() != 4 or pose.shape[-1] != 3:
        raise ValueError(f"egorear_amd.{what}: pose must be (N, T, J, 3), got {tuple(pose.shape)}")
    N, T, J = (int(v) for v in pose.shape[:3])
    if N < 1 or T < 1 or J < 1:
        raise ValueError(f"egorear_amd.{what}: empty pose {tuple(pose.shape)}")
    if T > TRAJECTORY_MAX_T:
        raise ValueError(f"egorear_amd.{what}: at most {TRAJECTORY_MAX_T} frames a clip are supported, got {T}")
    if N * T * J >= 1 << 31:
        raise ValueError(f"egorear_amd.{what}: N * T * J must stay below 2^31, got {tuple(pose.shape)}")
    if weight is not None and tuple(weight.shape) != (N, T, J):
        raise ValueError(f"egorear_amd.{what}: weight must be {(N, T, J)}, got {tuple(weight.shape)}")
    if obs is not None:
        _flags(what, obs, (N, T, J), "observed")
    _float32(what, (pose, "pose"), (weight, "weight"))
    _trajectory_parameters(what, vel_weight, accel_weight, huber, reweights, max_gap)
    _cotangents(what, (g_pose, (N, T, J, 3), "g_pose"))
    _contiguous(what, dense, (pose, "pose"), (weight, "weight"), (obs, "observed"), (g_pose, "g_pose"))
    return N, T, J


def trajectory_smooth(pose: torch.Tensor, weight: Optional[torch.Tensor] = None, obs: Optional[torch.Tensor] = None, vel_weight: float = 0.0,
                      accel_weight: float = 10.0, huber: float = 0.0, reweights: int = 0, max_gap: int = 8):
    """pose (N,T,J,3) cm, weight (N,T,J) | None (1), obs (N,T,J) u8 / bool | None (every frame) -> pose_out (N,T,J,3), valid (N,T,J) u8,
    residual (N,T,J), weight_out (N,T,J), energy (N,J): egr_trajectory_smooth_f32, the penalised least-squares trajectory of every joint
    of every clip (include/egorear_hip.h states the energy, the Huber reweighting and the validity rule).  The fp64 workspace of the
    elimination is allocated here, like the outputs."""
    N, T, J = _trajectory_operands(pose, weight, obs, vel_weight, accel_weight, huber, reweights, max_gap, "trajectory_smooth")
    _on_device("trajectory_smooth", pose, weight, obs)
    if obs is not None:
        obs = _flags("trajectory_smooth", obs, (N, T, J), "observed")
    dev = pose.device
    ws = torch.empty((TRAJECTORY_FWD_SLOTS, T, N * J), device=dev, dtype=torch.float64)
    pose_out = torch.empty((N, T, J, 3), device=dev, dtype=torch.float32)
    valid = torch.empty((N, T, J), device=dev, dtype=torch.uint8)
    residual, weight_out = (torch.empty((N, T, J), device=dev, dtype=torch.float32) for _ in range(2))
    energy = torch.empty((N, J), device=dev, dtype=torch.float32)
    sweeps = 2.0 * (reweights + 1)
    _launch("egr_trajectory_smooth_f32", lib.egr_trajectory_smooth_f32, _p(pose), _p(weight), _p(obs, torch.uint8), N, T, J, float(vel_weight),
            float(accel_weight), float(huber), int(reweights), int(max_gap), _p(ws, torch.float64), _p(pose_out), _p(valid, torch.uint8),
            _p(residual), _p(weight_out), _p(energy), _stream(), flops=N * T * J * sweeps * 40.0,
            nbytes=N * T * J * (sweeps * (40.0 + 17.0) + 21.0))
    return pose_out, valid, residual, weight_out, energy


def trajectory_smooth_bwd(pose: torch.Tensor, weight: Optional[torch.Tensor], obs: Optional[torch.Tensor], g_pose: torch.Tensor,
                          vel_weight: float = 0.0, accel_weight: float = 10.0):
    """Gradients of the plain form's pose_out with respect to pose and weight, (N,T,J,3) and (N,T,J) (None without a weight):
    egr_trajectory_smooth_bwd_f32 (the factorisation is recomputed from the operands)."""
    N, T, J = _trajectory_operands(pose, weight, obs, vel_weight, accel_weight, 0.0, 0, 0, "trajectory_smooth_bwd", g_pose)
    _on_device("trajectory_smooth_bwd", pose, weight, obs, g_pose)
    if obs is not None:
        obs = _flags("trajectory_smooth_bwd", obs, (N, T, J), "observed")
    dev = pose.device
    ws = torch.empty((TRAJECTORY_BWD_SLOTS, T, N * J), device=dev, dtype=torch.float64)
    g_in = torch.empty((N, T, J, 3), device=dev, dtype=torch.float32)
    g_weight = None if weight is None else torch.empty((N, T, J), device=dev, dtype=torch.float32)
    _launch("egr_trajectory_smooth_bwd_f32", lib.egr_trajectory_smooth_bwd_f32, _p(pose), _p(weight), _p(obs, torch.uint8), _p(g_pose), N, T, J,
            float(vel_weight), float(accel_weight), _p(ws, torch.float64), _p(g_in), _p(g_weight), _stream(), flops=N * T * J * 2.0 * 70.0,
            nbytes=N * T * J * (2.0 * 64.0 + 2.0 * 17.0 + 12.0 + 16.0))
    return g_in, g_weight


TRAJECTORY_FILTER_MAX_LAG = 64
TRAJECTORY_FILTER_HEAD_SLOTS, TRAJECTORY_FILTER_ROW_SLOTS = 23, 10      # fp64 state planes of N * J: the chain, two frames, two counts; a ring row


def trajectory_filter_state_slots(lag: int) -> int:
    if not _int_in(lag, 0, TRAJECTORY_FILTER_MAX_LAG):
        raise ValueError(f"egorear_amd.trajectory_filter: lag must be an integer in 0..{TRAJECTORY_FILTER_MAX_LAG}, got {lag!r}")
    return TRAJECTORY_FILTER_HEAD_SLOTS + TRAJECTORY_FILTER_ROW_SLOTS * lag


def _filter_parameters(what: str, N, J, lag, vel_weight, accel_weight, gate, max_gap) -> int:
    """The slot count of a filter state for N streams of J joints; every parameter error as ValueError."""
    if not (_int_in(N, 1, (1 << 31) - 1) and _int_in(J, 1, (1 << 31) - 1)):
        raise ValueError(f"egorear_amd.{what}: N and J must be positive integers, got {N!r}, {J!r}")
    if not _int_in(lag, 0, TRAJECTORY_FILTER_MAX_LAG):
        raise ValueError(f"egorear_amd.{what}: lag must be an integer in 0..{TRAJECTORY_FILTER_MAX_LAG}, got {lag!r}")
    _trajectory_parameters(what, vel_weight, accel_weight, 0.0, 0, max_gap)
    _non_negative(what, "gate", gate)
    slots = trajectory_filter_state_slots(lag)
    if N * J * slots >= 1 << 31:
        raise ValueError(f"egorear_amd.{what}: N * J * slots must stay below 2^31, got N {N}, J {J}, {slots} slots")
    return slots


def _filter_state(what: str, state, N: int, J: int, slots: int):
    if state.dtype != torch.float64 or tuple(state.shape) != (slots, N * J):
        raise ValueError(f"egorear_amd.{what}: state must be a float64 {(slots, N * J)} (trajectory_filter_state), got {state.dtype} "
                         f"{tuple(state.shape)}")
    if not state.is_contiguous():                        # (updated in place: a copy would not do, whoever calls)
        raise ValueError(f"egorear_amd.{what}: state must be contiguous")


def _filter_operands(state, pose, weight, obs, reset, lag, vel_weight, accel_weight, gate, max_gap, what: str, dense: bool = True):
    """(N, C, J) of a filter launch; every shape / dtype / parameter error as ValueError."""
    N, C, J = _trajectory_operands(pose, weight, obs, vel_weight, accel_weight, 0.0, 0, max_gap, what, dense=dense)
    slots = _filter_parameters(what, N, J, lag, vel_weight, accel_weight, gate, max_gap)
    _filter_state(what, state, N, J, slots)
    if reset is not None:
        _flags(what, reset, (N,), "reset")
        _contiguous(what, dense, (reset, "reset"))
    return N, C, J


def trajectory_filter_state(N: int, J: int, lag: int, device) -> torch.Tensor:
    """The empty state of N streams of J joints at `lag`: zeros (slots, N * J) float64 (include/egorear_hip.h has the layout)."""
    slots = _filter_parameters("trajectory_filter_state", N, J, lag, 0.0, 1.0, 0.0, 0)
    if torch.device(device).type not in ("cuda", "meta"):
        raise ValueError("egorear_amd.trajectory_filter_state: no CPU path - the state lives on the HIP device")
    return torch.zeros((slots, N * J), device=device, dtype=torch.float64)


def _filter_outputs(N: int, R: int, J: int, dev):
    pose_out = torch.empty((N, R, J, 3), device=dev, dtype=torch.float32)
    valid = torch.empty((N, R, J), device=dev, dtype=torch.uint8)
    residual, weight_out = (torch.empty((N, R, J), device=dev, dtype=torch.float32) for _ in range(2))
    frame = torch.empty((N, R), device=dev, dtype=torch.int64)
    return pose_out, valid, residual, weight_out, frame


def trajectory_filter(state: torch.Tensor, pose: torch.Tensor, weight: Optional[torch.Tensor] = None, obs: Optional[torch.Tensor] = None,
                      reset: Optional[torch.Tensor] = None, lag: int = 0, vel_weight: float = 0.0, accel_weight: float = 10.0,
                      gate: float = 0.0, max_gap: int = 8):
    """state (slots, N*J) f64, updated in place; pose (N,C,J,3) cm: the next C frames of N streams; weight (N,C,J) | None, obs (N,C,J) u8 /
    bool | None, reset (N,) u8 / bool | None -> pose_out (N,C,J,3), valid (N,C,J) u8, residual, weight_out (N,C,J), frame (N,C) int64:
    egr_trajectory_filter_f32, the causal fixed-lag form of trajectory_smooth - row c describes stream frame `frame[n, c]`, `lag` frames
    behind the arriving one (-1 and zeros before the stream is that long)."""
    N, C, J = _filter_operands(state, pose, weight, obs, reset, lag, vel_weight, accel_weight, gate, max_gap, "trajectory_filter")
    _on_device("trajectory_filter", state, pose, weight, obs, reset)
    if obs is not None:
        obs = _flags("trajectory_filter", obs, (N, C, J), "observed")
    if reset is not None:
        reset = _flags("trajectory_filter", reset, (N,), "reset")
    out = _filter_outputs(N, C, J, pose.device)
    _launch("egr_trajectory_filter_f32", lib.egr_trajectory_filter_f32, _p(pose), _p(weight), _p(obs, torch.uint8), _p(reset, torch.uint8),
            _p(state, torch.float64), N, C, J, int(lag), float(vel_weight), float(accel_weight), float(gate), int(max_gap), _p(out[0]),
            _p(out[1], torch.uint8), _p(out[2]), _p(out[3]), _p(out[4], torch.int64), _stream(), flops=N * C * J * (160.0 + 20.0 * lag),
            nbytes=N * J * (2.0 * 8.0 * TRAJECTORY_FILTER_HEAD_SLOTS + C * (17.0 + 21.0 + 80.0 + 48.0 * lag)))
    return out


def trajectory_filter_tail(state: torch.Tensor, N: int, J: int, lag: int, vel_weight: float = 0.0, accel_weight: float = 10.0,
                           max_gap: int = 8):
    """state (slots, N*J) f64, read only -> pose_out (N,lag,J,3), valid (N,lag,J) u8, residual, weight_out (N,lag,J), frame (N,lag) int64:
    egr_trajectory_filter_tail_f32, the last `lag` frames of the stream so far, which no arrival has described yet (rows before the
    stream's start: -1 and zeros).  The last row is the causal estimate of the present."""
    slots = _filter_parameters("trajectory_filter_tail", N, J, lag, vel_weight, accel_weight, 0.0, max_gap)
    _filter_state("trajectory_filter_tail", state, N, J, slots)
    _on_device("trajectory_filter_tail", state)
    out = _filter_outputs(N, lag, J, state.device)
    if lag > 0:
        _launch("egr_trajectory_filter_tail_f32", lib.egr_trajectory_filter_tail_f32, _p(state, torch.float64), N, J, int(lag),
                float(vel_weight), float(accel_weight), int(max_gap), _p(out[0]), _p(out[1], torch.uint8), _p(out[2]), _p(out[3]),
                _p(out[4], torch.int64), _stream(), flops=N * J * (80.0 + 20.0 * lag), nbytes=N * J * lag * (80.0 + 21.0))
    return out


RAY_TRACK_RAY_SLOTS, RAY_TRACK_SOLVE_SLOTS = 4, 18    # fp64 workspace planes of T * N * J: d[3], w a view; E (9), D^-1 (6), q (3)


def _ray_track_operands(coords, conf, cams, ctm, sx, sy, threshold, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio,
                        what: str, dense: bool = True):
    """(N, T, V, J) of a ray-track launch; every shape / dtype / parameter error as ValueError."""
    if coords.dim() != 5 or coords.shape[-1] != 2:
        raise ValueError(f"egorear_amd.{what}: coords must be (N, T, V, J, 2), got {tuple(coords.shape)}")
    N, T, V, J = (int(v) for v in coords.shape[:4])
    if N < 1 or T < 1 or J < 1:
        raise ValueError(f"egorear_amd.{what}: empty coords {tuple(coords.shape)}")
    if T > TRAJECTORY_MAX_T:
        raise ValueError(f"egorear_amd.{what}: at most {TRAJECTORY_MAX_T} frames a clip are supported, got {T}")
    if tuple(conf.shape) != (N, T, V, J):
        raise ValueError(f"egorear_amd.{what}: conf must be {(N, T, V, J)}, got {tuple(conf.shape)}")
    if not 2 <= V <= 4:
        raise ValueError(f"egorear_amd.{what}: 2 to 4 views are supported, got {V}")
    if tuple(cams.shape) != (V, RAY_REC):
        raise ValueError(f"egorear_amd.{what}: cams must be {(V, RAY_REC)} (camera.packed_rays()), got {tuple(cams.shape)}")
    if ctm is not None and tuple(ctm.shape) != (N, T, V, 4, 4):
        raise ValueError(f"egorear_amd.{what}: coord_trans_mat must be {(N, T, V, 4, 4)}, got {tuple(ctm.shape)}")
    if N * T * V * J * 2 >= 1 << 31:
        raise ValueError(f"egorear_amd.{what}: N * T * V * J * 2 must stay below 2^31, got {tuple(coords.shape)}")
    _float32(what, (coords, "coords"), (conf, "conf"), (cams, "cams"), (ctm, "coord_trans_mat"))
    _positive(what, "the coordinate scales", sx, sy)
    if not (isinstance(threshold, (int, float)) and not isinstance(threshold, bool) and threshold == threshold):
        raise ValueError(f"egorear_amd.{what}: threshold must be a number, got {threshold!r}")
    _trajectory_parameters(what, vel_weight, accel_weight, huber, reweights, max_gap)
    if not (isinstance(min_pivot_ratio, (int, float)) and not isinstance(min_pivot_ratio, bool) and 0.0 <= min_pivot_ratio < 1.0):
        raise ValueError(f"egorear_amd.{what}: min_pivot_ratio must be a number in [0, 1), got {min_pivot_ratio!r}")
    _contiguous(what, dense, (coords, "coords"), (conf, "conf"), (cams, "cams"), (ctm, "coord_trans_mat"))
    return N, T, V, J


def ray_track(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor] = None, sx: float = 1.0,
              sy: float = 1.0, threshold: float = 0.5, vel_weight: float = 0.0, accel_weight: float = 10.0, huber: float = 0.0,
              reweights: int = 0, max_gap: int = 8, min_pivot_ratio: float = 1e-10):
    """coords (N,T,V,J,2), conf (N,T,V,J), cams (V,30) = camera.packed_rays(), ctm (N,T,V,4,4) | None (the syn rig) -> pose (N,T,J,3) cm,
    valid (N,T,J) u8, residual (N,T,V,J) cm, weight (N,T,V,J), rays (N,T,J) u8, energy (N,J): egr_ray_track_f32, per joint of every clip
    the track that is closest to the views' rays over the frames under a velocity and an acceleration penalty (include/egorear_hip.h
    states the energy, the Huber reweighting, the solvability and the validity rule).  The fp64 workspace is allocated here, like the
    outputs.  Two launches behind the one entry."""
    N, T, V, J = _ray_track_operands(coords, conf, cams, ctm, sx, sy, threshold, vel_weight, accel_weight, huber, reweights, max_gap,
                                     min_pivot_ratio, "ray_track")
    _on_device("ray_track", coords, conf, cams, ctm)
    dev = coords.device
    nbytes_ws = int(lib.egr_ray_track_workspace_bytes(N, T, V, J))
    ws = torch.empty((nbytes_ws // 8,), device=dev, dtype=torch.float64)
    pose = torch.empty((N, T, J, 3), device=dev, dtype=torch.float32)
    valid, rays = (torch.empty((N, T, J), device=dev, dtype=torch.uint8) for _ in range(2))
    residual, weight = (torch.empty((N, T, V, J), device=dev, dtype=torch.float32) for _ in range(2))
    energy = torch.empty((N, J), device=dev, dtype=torch.float32)
    solves = reweights + 1.0
    _launch("egr_ray_track_f32", lib.egr_ray_track_f32, _p(coords), _p(conf), _p(cams), _p(ctm), N, T, V, J, float(sx), float(sy),
            float(threshold), float(vel_weight), float(accel_weight), float(huber), int(reweights), int(max_gap), float(min_pivot_ratio),
            _p(ws, torch.float64), nbytes_ws, _p(pose), _p(valid, torch.uint8), _p(residual), _p(weight), _p(rays, torch.uint8), _p(energy),
            _stream(), flops=N * T * J * (solves * (V * 90.0 + 330.0) + V * 60.0),
            nbytes=N * T * J * (V * (12.0 + 32.0) + solves * (V * 32.0 + 3.0 * 144.0 + 24.0) + V * 40.0 + 38.0))
    return pose, valid, residual, weight, rays, energy


INFO_TRACK_SOLVE_SLOTS = 18       # fp64 workspace planes of T * N * J of egr_infotrack.hip: E (9), D^-1 (6), q (3)


def _joint_info_operands(points, conf, cams, ctm, sx, sy, threshold, min_det_ratio, what: str, dense: bool = True):
    """(B, V, J) of a joint-information launch; every shape / dtype / parameter error as ValueError."""
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"egorear_amd.{what}: points must be (B, J, 3), got {tuple(points.shape)}")
    B, J = int(points.shape[0]), int(points.shape[1])
    if B < 1 or J < 1:
        raise ValueError(f"egorear_amd.{what}: empty points {tuple(points.shape)}")
    if conf.dim() != 3 or (int(conf.shape[0]), int(conf.shape[2])) != (B, J):
        raise ValueError(f"egorear_amd.{what}: conf must be ({B}, V, {J}), got {tuple(conf.shape)}")
    V = int(conf.shape[1])
    _rig(what, cams, ctm, B, V)
    if B * J * V >= 1 << 30:
        raise ValueError(f"egorear_amd.{what}: B * J * V must stay below 2^30, got {tuple(conf.shape)}")
    _float32(what, (points, "points"), (conf, "conf"), (cams, "cams"), (ctm, "coord_trans_mat"))
    _positive(what, "the coordinate scales", sx, sy)
    if not (isinstance(threshold, (int, float)) and not isinstance(threshold, bool) and threshold == threshold):
        raise ValueError(f"egorear_amd.{what}: threshold must be a number, got {threshold!r}")
    _non_negative(what, "min_det_ratio", min_det_ratio)
    _contiguous(what, dense, (points, "points"), (conf, "conf"), (cams, "cams"), (ctm, "coord_trans_mat"))
    return B, V, J


def joint_info(points: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor] = None, sx: float = 1.0,
               sy: float = 1.0, threshold: float = 0.5, min_det_ratio: float = 1e-6):
    """points (B,J,3) cm, conf (B,V,J), cams (V,30) = camera.packed_rays(), ctm (B,V,4,4) | None (the syn rig) -> info (B,J,6), views
    (B,J) u8, sigma (B,J), valid (B,J) u8: egr_joint_info_f32, the 3 x 3 information matrix sum_v conf_v J_v^T J_v of the views'
    reprojections at every point (include/egorear_hip.h states which views enter and what sigma and valid are)."""
    B, V, J = _joint_info_operands(points, conf, cams, ctm, sx, sy, threshold, min_det_ratio, "joint_info")
    _on_device("joint_info", points, conf, cams, ctm)
    dev = points.device
    info = torch.empty((B, J, 6), device=dev, dtype=torch.float32)
    sigma = torch.empty((B, J), device=dev, dtype=torch.float32)
    views, valid = (torch.empty((B, J), device=dev, dtype=torch.uint8) for _ in range(2))
    _launch("egr_joint_info_f32", lib.egr_joint_info_f32, _p(points), _p(conf), _p(cams), _p(ctm), B, V, J, float(sx), float(sy),
            float(threshold), float(min_det_ratio), _p(info), _p(views, torch.uint8), _p(sigma), _p(valid, torch.uint8), _stream(),
            flops=B * J * (V * 150.0 + 60.0), nbytes=B * J * (V * (4.0 + (64.0 if ctm is not None else 0.0)) + 12.0 + 30.0))
    return info, views, sigma, valid


def _info_track_operands(pose, info, obs, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio, what: str, dense: bool = True):
    """(N, T, J) of an information-track launch; every shape / dtype / parameter error as ValueError."""
    if pose.dim() != 4 or pose.shape[-1] != 3:
        raise ValueError(f"egorear_amd.{what}: pose must be (N, T, J, 3), got {tuple(pose.shape)}")
    N, T, J = (int(v) for v in pose.shape[:3])
    if N < 1 or T < 1 or J < 1:
        raise ValueError(f"egorear_amd.{what}: empty pose {tuple(pose.shape)}")
    if T > TRAJECTORY_MAX_T:
        raise ValueError(f"egorear_amd.{what}: at most {TRAJECTORY_MAX_T} frames a clip are supported, got {T}")
    if tuple(info.shape) != (N, T, J, 6):
        raise ValueError(f"egorear_amd.{what}: info must be {(N, T, J, 6)}, got {tuple(info.shape)}")
    if N * T * J * 6 >= 1 << 31:
        raise ValueError(f"egorear_amd.{what}: N * T * J * 6 must stay below 2^31, got {tuple(pose.shape)}")
    if obs is not None:
        _flags(what, obs, (N, T, J), "observed")
    _float32(what, (pose, "pose"), (info, "info"))
    _trajectory_parameters(what, vel_weight, accel_weight, huber, reweights, max_gap)
    if not (isinstance(min_pivot_ratio, (int, float)) and not isinstance(min_pivot_ratio, bool) and 0.0 <= min_pivot_ratio < 1.0):
        raise ValueError(f"egorear_amd.{what}: min_pivot_ratio must be a number in [0, 1), got {min_pivot_ratio!r}")
    _contiguous(what, dense, (pose, "pose"), (info, "info"), (obs, "observed"))
    return N, T, J


def info_track(pose: torch.Tensor, info: torch.Tensor, obs: Optional[torch.Tensor] = None, vel_weight: float = 0.0, accel_weight: float = 1.0,
               huber: float = 0.0, reweights: int = 0, max_gap: int = 8, min_pivot_ratio: float = 1e-10):
    """pose (N,T,J,3) cm, info (N,T,J,6) = joint_info's matrices, obs (N,T,J) u8 / bool | None (every frame) -> pose_out (N,T,J,3),
    valid (N,T,J) u8, residual (N,T,J) in coordinate units, weight (N,T,J), energy (N,J): egr_info_track_f32, the clip smoother whose
    data term is (x - z)^T W (x - z) a frame (include/egorear_hip.h states the energy, the Huber reweighting in pixels, the solvability
    and the validity rule).  The fp64 workspace is allocated here, like the outputs.  One launch."""
    N, T, J = _info_track_operands(pose, info, obs, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio, "info_track")
    _on_device("info_track", pose, info, obs)
    if obs is not None:
        obs = _flags("info_track", obs, (N, T, J), "observed")
    dev = pose.device
    nbytes_ws = int(lib.egr_info_track_workspace_bytes(N, T, J))
    ws = torch.empty((nbytes_ws // 8,), device=dev, dtype=torch.float64)
    pose_out = torch.empty((N, T, J, 3), device=dev, dtype=torch.float32)
    valid = torch.empty((N, T, J), device=dev, dtype=torch.uint8)
    residual, weight = (torch.empty((N, T, J), device=dev, dtype=torch.float32) for _ in range(2))
    energy = torch.empty((N, J), device=dev, dtype=torch.float32)
    solves = reweights + 1.0
    _launch("egr_info_track_f32", lib.egr_info_track_f32, _p(pose), _p(info), _p(obs, torch.uint8), N, T, J, float(vel_weight),
            float(accel_weight), float(huber), int(reweights), int(max_gap), float(min_pivot_ratio), _p(ws, torch.float64), nbytes_ws,
            _p(pose_out), _p(valid, torch.uint8), _p(residual), _p(weight), _p(energy), _stream(),
            flops=N * T * J * (solves * 360.0 + 40.0), nbytes=N * T * J * (solves * (37.0 + 3.0 * 144.0 + 24.0) + 37.0 + 24.0 + 21.0))
    return pose_out, valid, residual, weight, energy


def layernorm(x: torch.Tensor, gamma, beta, res: Optional[torch.Tensor] = None, eps: float = 1e-5, groups: int = 1) -> torch.Tensor:
    _cont(x, "layernorm input")
    c = x.shape[-1]
    rows = x.numel() // c
    if res is not None and (res.shape != x.shape or not res.is_contiguous()):
        raise RuntimeError("egorear_amd.layernorm: residual must match the input")
    if gamma.numel() != groups * c or beta.numel() != groups * c or rows % groups:
        raise RuntimeError("egorear_amd.layernorm: gamma/beta/groups mismatch")
    y = torch.empty_like(x)
    _launch("egr_layernorm_f32", lib.egr_layernorm_f32, _p(x), _p(res), _p(gamma), _p(beta), _p(y), rows, c, eps,
            rows // groups if groups > 1 else 0, _stream(), nbytes=4.0 * rows * c * (3 if res is not None else 2))
    return y


def joint_mha(qkv: torch.Tensor, b: int, j: int, heads: int, d: int, scale: float) -> torch.Tensor:
    _cont(qkv, "qkv")
    if qkv.numel() != b * j * 3 * heads * d:
        raise RuntimeError("egorear_amd.joint_mha: qkv size mismatch")
    out = torch.empty((b * j, heads * d), device=qkv.device, dtype=torch.float32)
    _launch("egr_joint_mha_f32", lib.egr_joint_mha_f32, _p(qkv), _p(out), b, j, heads, d, float(scale), _stream())
    return out


def msda_gather(feat: torch.Tensor, pos: Optional[torch.Tensor], offs_logits: torch.Tensor, anchors: torch.Tensor,
                valid: torch.Tensor, b: int, views: int, joints: int, heads: int, dh: int, hgt: int, wid: int, groups: int = 1):
    """feat (views, b, hgt*wid, cf) contiguous.  Returns g (G, rows, heads, cf), e (G, rows, heads*dh) | None,
    sigma (G, heads, rows), rowmask (rows,) with rows = (b, joint, view); G query sets (offs_logits (G, b*joints, .),
    pos (G, views, hgt*wid, heads*dh)) share feat / anchors / valid."""
    _cont(feat, "feature memory"); _cont(offs_logits, "offs_logits"); _cont(anchors, "anchors"); _cont(valid, "valid")
    cf = feat.shape[-1]
    if feat.numel() != views * b * hgt * wid * cf:
        raise RuntimeError("egorear_amd.msda_gather: feature memory size mismatch")
    if offs_logits.numel() != groups * b * joints * heads * 16 * 3:
        raise RuntimeError("egorear_amd.msda_gather: offs_logits size mismatch")
    if anchors.numel() != b * views * joints * 2 or valid.numel() != b * views * joints:
        raise RuntimeError("egorear_amd.msda_gather: anchors/valid size mismatch")
    if pos is not None:
        _cont(pos, "positional table")
        if pos.numel() != groups * views * hgt * wid * heads * dh:
            raise RuntimeError("egorear_amd.msda_gather: positional table size mismatch")
    rows = b * joints * views
    dev = feat.device
    g = torch.empty((groups, rows, heads, cf), device=dev, dtype=torch.float32)
    e = torch.empty((groups, rows, heads * dh), device=dev, dtype=torch.float32) if pos is not None else None
    sigma = torch.empty((groups, heads, rows), device=dev, dtype=torch.float32)
    rowmask = torch.empty((rows,), device=dev, dtype=torch.uint8)
    _launch("egr_msda_gather_f32", lib.egr_msda_gather_f32, _p(feat), cf, _p(pos), dh, _p(offs_logits), _p(anchors), _p(valid, torch.uint8), b, views,
                                   joints, heads, hgt, wid, _p(g), _p(e), _p(sigma), _p(rowmask, torch.uint8), groups, _stream(),
            # algorithmic bytes: 16 points x 4 bilinear corners x (cf + dh) floats per (query set, row, head) gathered (served
            # mostly by L2), the offsets / logits read, g / e / sigma written
            nbytes=4.0 * groups * rows * heads * (64.0 * (cf + (dh if pos is not None else 0)) + 48 + cf + (dh if pos is not None else 0) + 1),
            # unique bytes (what HBM must deliver at least: every operand once, every output once) for bench.py's roofline_hbm entry
            tag=("unique%d" % (4 * (feat.numel() + (pos.numel() if pos is not None else 0) + offs_logits.numel() + anchors.numel() + g.numel()
                                    + (e.numel() if e is not None else 0) + sigma.numel()) + valid.numel() + rowmask.numel())) if PROFILE is not None else "")
    return g, e, sigma, rowmask


def fisheye_project(pts: torch.Tensor, ctm: Optional[torch.Tensor], cams: torch.Tensor, out: Optional[torch.Tensor] = None):
    """pts (b, joints, 3) is updated IN PLACE in syn mode (ctm None), as the reference does - or, with `out`,
    left alone and the updated points (syn: mutated, rw: a copy) written there."""
    _cont(pts, "pts")
    b, joints = pts.shape[:2]
    if cams.numel() != 4 * 17:
        raise RuntimeError("egorear_amd.fisheye_project: cams must hold 4 records of 17 floats")
    if ctm is not None:
        _cont(ctm, "coord_trans_mat")
        if ctm.numel() != b * 4 * 16:
            raise RuntimeError("egorear_amd.fisheye_project: coord_trans_mat must be (b,4,4,4)")
    dev = pts.device
    anchors = torch.empty((b, 4, joints, 2), device=dev, dtype=torch.float32)
    valid = torch.empty((b, 4, joints), device=dev, dtype=torch.uint8)
    q4 = torch.empty((b * joints, 4), device=dev, dtype=torch.float32)
    if out is not None:
        if out.shape != pts.shape or not out.is_contiguous():
            raise RuntimeError("egorear_amd.fisheye_project: out must be a contiguous tensor of pts' shape")
        _launch("egr_fisheye_project_f32", lib.egr_fisheye_project2_f32, _p(pts), _p(out), _p(ctm), _p(cams), b, joints, _p(anchors),
                _p(valid, torch.uint8), _p(q4), _stream())
        return anchors, valid, q4
    _launch("egr_fisheye_project_f32", lib.egr_fisheye_project_f32, _p(pts), _p(ctm), _p(cams), b, joints, _p(anchors), _p(valid, torch.uint8), _p(q4),
                                       _stream())
    return anchors, valid, q4


def linear_smallk(x: torch.Tensor, sxm: int, sxk: int, w: torch.Tensor, bias, m: int, n: int, k: int, act: int,
                  groups: int = 1) -> torch.Tensor:
    _cont(w, "weight")
    if w.numel() != groups * n * k or m % groups or (m - 1) * sxm + (k - 1) * sxk >= x.numel():
        raise RuntimeError("egorear_amd.linear_smallk: size mismatch")
    y = torch.empty((m, n), device=x.device, dtype=torch.float32)
    _launch("egr_linear_smallk_f32", lib.egr_linear_smallk_f32, _p(x), sxm, sxk, _p(w), _p(bias), _p(y), m, n, k, act,
            m // groups if groups > 1 else 0, _stream())
    return y


def jqa_sum(hm_embed: torch.Tensor, embed: torch.Tensor, bfb: torch.Tensor, b: int, j: int, c: int, groups: int = 1) -> torch.Tensor:
    """b counts all frames of all groups (groups x frames per group); embed is (groups, j, c)."""
    _cont(hm_embed, "hm_embed"); _cont(embed, "embed"); _cont(bfb, "bfb")
    if hm_embed.numel() != b * j * c or embed.numel() != groups * j * c or bfb.numel() != b * c or b % groups:
        raise RuntimeError("egorear_amd.jqa_sum: size mismatch")
    y = torch.empty((b * j, c), device=hm_embed.device, dtype=torch.float32)
    _launch("egr_jqa_sum_f32", lib.egr_jqa_sum_f32, _p(hm_embed), _p(embed), _p(bfb), _p(y), b, j, c,
            b // groups if groups > 1 else 0, _stream())
    return y


def tokens_to_nhwc(x: torch.Tensor, b: int, j: int, hw: int) -> torch.Tensor:
    _cont(x, "tokens")
    if x.numel() != b * j * hw:
        raise RuntimeError("egorear_amd.tokens_to_nhwc: size mismatch")
    y = torch.empty((b, hw, j), device=x.device, dtype=torch.float32)
    _launch("egr_tokens_to_nhwc_f32", lib.egr_tokens_to_nhwc_f32, _p(x), _p(y), b, j, hw, _stream())
    return y


def pack_layer_w(w: torch.Tensor) -> torch.Tensor:
    """(..., rows, k) fp32 weight stack -> the same shape in egr_joint_layer_f32's fragment order (egr_pack_layer_w_f32)."""
    rows, k = w.shape[-2], w.shape[-1]
    if w.dtype != torch.float32 or rows % 16 or k % 128:
        raise RuntimeError("egorear_amd.pack_layer_w: fp32, rows % 16 == 0, k % 128 == 0 expected")
    w = _cont(w, "layer weight")
    out = torch.empty_like(w)
    _launch("egr_pack_layer_w_f32", lib.egr_pack_layer_w_f32, _p(w), w.numel() // (rows * k), rows, k, _p(out), _stream())
    return out


def pack_layer_wh2(w: torch.Tensor) -> torch.Tensor:
    """(..., rows, k) fp32 weight stack -> (..., rows * k + rows) floats: per matrix the fp16-scheme image egr_joint_layer_f32 reads with
    w_packed = 2 (two fp16 planes per weight in fragment order) and the rows' descales behind it (egr_pack_layer_wh2_f32)."""
    rows, k = w.shape[-2], w.shape[-1]
    if w.dtype != torch.float32 or rows % 16 or k % 128:
        raise RuntimeError("egorear_amd.pack_layer_wh2: fp32, rows % 16 == 0, k % 128 == 0 expected")
    w = _cont(w, "layer weight")
    out = torch.empty(w.shape[:-2] + (rows * k + rows,), device=w.device, dtype=torch.float32)
    _launch("egr_pack_layer_wh2_f32", lib.egr_pack_layer_wh2_f32, _p(w), w.numel() // (rows * k), rows, k, _p(out), _stream())
    return out


def joint_layer(x: torch.Tensor, g: torch.Tensor, e: Optional[torch.Tensor], sigma: torch.Tensor, rowmask: torch.Tensor, W: dict,
                B: int, J: int, V: int, Cdim: int, groups: int, *, ol: Optional[dict] = None, post: Optional[dict] = None,
                reg: Optional[dict] = None, want_xn: bool = False, head: Optional[dict] = None):
    """One transformer layer behind egr_msda_gather_f32 as one launch (egr_joint_layer_f32).  W: the layer's plain weight stacks
    (engine.pack_layer_fused).  ol = {"w", "b"}: also the next layer's offsets / logits; post = {"g", "b"}: also post_norm
    (want_xn: return it); reg = {"w0", "b0", "w2", "b2", "anchors"}: also the 3-D regression head; head = {"w" (groups, 64, J),
    "b" (groups, 64), "amax": record | None}: also the refiner's head offset (tokens as a 16 x 16 image -> 1x1 conv + ReLU -> up x2),
    returned as head["out"] (groups*B, 32, 32, 64).
    Returns (x_out, ol_out | None, xn | None, pred | None)."""
    rows = groups * B * J
    if x.shape != (rows, Cdim) or not x.is_contiguous():
        raise RuntimeError("egorear_amd.joint_layer: x must be (groups*B*J, C) contiguous")
    if g.numel() != groups * B * J * V * 4 * 128 or sigma.numel() != groups * 4 * B * J * V or rowmask.numel() != B * J * V:
        raise RuntimeError("egorear_amd.joint_layer: sampled operands do not match (B, J, V)")
    if e is not None and e.numel() != groups * B * J * V * Cdim:
        raise RuntimeError("egorear_amd.joint_layer: e does not match")
    packed = W.get("packed")
    packed = 2 if packed == 2 else (1 if packed else 0)     # 2: the fp16-scheme images (pack_layer_wh2), 1: fragment order (pack_layer_w)

    def msz(rows, k):                                       # floats of one weight matrix as passed
        return rows * k + (rows if packed == 2 else 0)
    need = {"w_fold": groups * msz(Cdim, 128), "c_fold": groups * Cdim, "w_out": groups * msz(Cdim, Cdim), "b_out": groups * Cdim,
            "w_fuse": groups * msz(Cdim, V * Cdim), "b_fuse": groups * Cdim, "ln1_g": groups * Cdim, "ln1_b": groups * Cdim,
            "w_qkv": groups * msz(3 * Cdim, Cdim), "b_qkv": groups * 3 * Cdim, "w_mo": groups * msz(Cdim, Cdim), "b_mo": groups * Cdim,
            "ln2_g": groups * Cdim, "ln2_b": groups * Cdim, "w_f0": groups * msz(512, Cdim), "b_f0": groups * 512,
            "w_f1": groups * msz(Cdim, 512), "b_f1": groups * Cdim, "ln3_g": groups * Cdim, "ln3_b": groups * Cdim}
    d = LayerDesc()
    d.B, d.J, d.V, d.C, d.heads, d.cf, d.groups, d.ffn_dim = B, J, V, Cdim, 4, 128, groups, 512
    d.eps, d.mha_scale = 1e-5, float((Cdim // 4) ** -0.5)
    d.x, d.g, d.e, d.sigma, d.rowmask = _p(x), _p(_cont(g, "g")), _p(e), _p(_cont(sigma, "sigma")), _p(rowmask, torch.uint8)
    for k, n in need.items():
        t = W[k]
        if t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"egorear_amd.joint_layer: weight {k} has {t.numel()} elements, expected {n}")
        setattr(d, k, _p(t))
    d.w_packed = packed                          # the matrices of W, ol and reg are then all in that order
    x_out = torch.empty_like(x)
    d.x_out = _p(x_out)
    ol_out = xn = pred = None
    if ol is not None:
        n = ol["b"].shape[-1]
        if ol["w"].numel() != groups * msz(n, Cdim) or ol["b"].numel() != groups * n or n % 16:
            raise RuntimeError("egorear_amd.joint_layer: offsets / logits weights do not match")
        ol_out = torch.empty((rows, n), device=x.device, dtype=torch.float32)
        d.w_ol, d.b_ol, d.ol_out, d.ol_n = _p(_cont(ol["w"], "w_ol")), _p(ol["b"]), _p(ol_out), n
    if post is not None:
        if post["g"].numel() != groups * Cdim or post["b"].numel() != groups * Cdim:
            raise RuntimeError("egorear_amd.joint_layer: post_norm parameters do not match")
        d.lnp_g, d.lnp_b = _p(post["g"]), _p(post["b"])
        if want_xn:
            xn = torch.empty_like(x)
            d.xn_out = _p(xn)
    if reg is not None:
        if post is None:
            raise RuntimeError("egorear_amd.joint_layer: the regression head sits behind post_norm")
        if reg["w0"].numel() != groups * msz(Cdim, Cdim) or reg["w2"].numel() != groups * 3 * Cdim or reg["anchors"].numel() != rows * 3:
            raise RuntimeError("egorear_amd.joint_layer: regression head operands do not match")
        pred = torch.empty((rows, 3), device=x.device, dtype=torch.float32)
        d.w_r0, d.b_r0, d.w_r2, d.b_r2 = _p(_cont(reg["w0"], "w_r0")), _p(reg["b0"]), _p(_cont(reg["w2"], "w_r2")), _p(reg["b2"])
        d.anchors3d, d.pred_out = _p(_cont(reg["anchors"], "anchors")), _p(pred)
    if head is not None:
        if post is None or reg is not None or Cdim != 256:
            raise RuntimeError("egorear_amd.joint_layer: the head offset sits behind post_norm of a 256-channel layer, without the regression head")
        hn = head["b"].shape[-1]
        if hn != 64 or head["w"].numel() != groups * hn * J or head["b"].numel() != groups * hn:
            raise RuntimeError("egorear_amd.joint_layer: head offset weights do not match")
        h0 = torch.empty((groups * B, 32, 32, hn), device=x.device, dtype=torch.float32)
        d.w_h0, d.b_h0, d.h0_out, d.h0_n = _p(_cont(head["w"], "w_h0")), _p(_cont(head["b"], "b_h0")), _p(h0), hn
        rec = head.get("amax")
        if rec is not None:
            d.amax_h0 = _p(rec, torch.int32)
            h0._egr_amax = rec
        head["out"] = h0
    flops = 2.0 * groups * B * (J * V * (Cdim * 128 + Cdim * Cdim) + J * (V * Cdim * Cdim + 3 * Cdim * Cdim + Cdim * Cdim + 2 * 512 * Cdim))
    _launch("egr_joint_layer_f32", lib.egr_joint_layer_f32, C.byref(d), _stream(), flops=flops,
            tag=f"{'h2' if packed == 2 else 'plain'} G{groups} B{B} J{J} C{Cdim}" if PROFILE is not None else "")
    return x_out, ol_out, xn, pred


def jqa_query(t: torch.Tensor, s32: torch.Tensor, W: dict, B: int, J: int, Cdim: int, groups: int):
    """The JQA query of the refiners as one launch (egr_jqa_query_f32): t (groups*B*J, C) = ReLU(heatmap_proj[0](hm)), s32
    (groups*B, h, w, 512) NHWC.  W: {"w_hp2", "b_hp2", "w_bfb", "b_bfb", "embed", "w_q", "b_q", "w_ol", "b_ol", "packed"} - matrices in
    pack_layer_w / pack_layer_wh2 order.  Returns (x (groups*B*J, C), ol (groups*B*J, ol_n))."""
    rows = groups * B * J
    if t.shape != (rows, Cdim) or not t.is_contiguous() or Cdim != 256:
        raise RuntimeError("egorear_amd.jqa_query: t must be (groups*B*J, 256) contiguous")
    if s32.dim() != 4 or s32.shape[0] != groups * B or s32.shape[3] != 512 or not s32.is_contiguous():
        raise RuntimeError("egorear_amd.jqa_query: s32 must be (groups*B, h, w, 512) contiguous NHWC")
    packed = W.get("packed")
    packed = 2 if packed == 2 else (1 if packed else 0)

    def msz(r, k):
        return r * k + (r if packed == 2 else 0)
    n = W["b_ol"].shape[-1]
    need = {"w_hp2": groups * msz(Cdim, Cdim), "b_hp2": groups * Cdim, "w_bfb": groups * msz(Cdim, 512), "b_bfb": groups * Cdim,
            "embed": groups * J * Cdim, "w_q": groups * msz(Cdim, Cdim), "b_q": groups * Cdim, "w_ol": groups * msz(n, Cdim), "b_ol": groups * n}
    d = JqaQueryDesc()
    d.B, d.J, d.C, d.groups, d.kb, d.pool_hw, d.ol_n, d.w_packed = B, J, Cdim, groups, 512, s32.shape[1] * s32.shape[2], n, packed
    d.t, d.s32 = _p(t), _p(s32)
    for k, ne in need.items():
        w = W[k]
        if w.numel() != ne or not w.is_contiguous():
            raise RuntimeError(f"egorear_amd.jqa_query: weight {k} has {w.numel()} elements, expected {ne}")
        setattr(d, k, _p(w))
    x = torch.empty((rows, Cdim), device=t.device, dtype=torch.float32)
    ol = torch.empty((rows, n), device=t.device, dtype=torch.float32)
    d.x_out, d.ol_out = _p(x), _p(ol)
    _launch("egr_jqa_query_f32", lib.egr_jqa_query_f32, C.byref(d), _stream(),
            flops=2.0 * groups * B * (J * Cdim * (2 * Cdim + n) + Cdim * 512))
    return x, ol


def pose_query(h1: torch.Tensor, ctm: Optional[torch.Tensor], cams: torch.Tensor, W: dict, B: int, J: int, Cdim: int):
    """The lifting head between mlp_pred[1] and its first decoder layer as one launch (egr_pose_query_f32).  h1 (B, C).  W: {"w_m2",
    "b_m2", "w_qg0", "b_qg0", "w_qg2", "b_qg2", "w_qg4", "b_qg4", "w_ol", "b_ol", "packed"}.
    Returns (pred (B, J, 3), anchors_3d (B, J, 3), anchors_2d (B, 4, J, 2), valid (B, 4, J) uint8, x (B*J, C), ol (B*J, ol_n))."""
    if h1.shape != (B, Cdim) or not h1.is_contiguous() or Cdim != 128 or J != 16:
        raise RuntimeError("egorear_amd.pose_query: h1 must be (B, 128) contiguous, 16 joints")
    if ctm is not None and (ctm.shape != (B, 4, 4, 4) or not ctm.is_contiguous()):
        raise RuntimeError("egorear_amd.pose_query: coord_trans_mat must be (B, 4, 4, 4) contiguous")
    packed = W.get("packed")
    packed = 2 if packed == 2 else (1 if packed else 0)

    def msz(r, k):
        return r * k + (r if packed == 2 else 0)
    n = W["b_ol"].shape[-1]
    need = {"w_m2": msz(3 * J, Cdim), "b_m2": 3 * J, "w_qg0": Cdim * 4, "b_qg0": Cdim, "w_qg2": msz(Cdim, Cdim), "b_qg2": Cdim,
            "w_qg4": msz(Cdim, Cdim), "b_qg4": Cdim, "w_ol": msz(n, Cdim), "b_ol": n}
    d = PoseQueryDesc()
    d.B, d.J, d.C, d.ol_n, d.w_packed = B, J, Cdim, n, packed
    d.h1, d.ctm, d.cams = _p(h1), _p(ctm), _p(cams)
    for k, ne in need.items():
        w = W[k]
        if w.numel() != ne or not w.is_contiguous():
            raise RuntimeError(f"egorear_amd.pose_query: weight {k} has {w.numel()} elements, expected {ne}")
        setattr(d, k, _p(w))
    dev = h1.device
    pred = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
    a3 = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
    a2 = torch.empty((B, 4, J, 2), device=dev, dtype=torch.float32)
    valid = torch.empty((B, 4, J), device=dev, dtype=torch.uint8)
    x = torch.empty((B * J, Cdim), device=dev, dtype=torch.float32)
    ol = torch.empty((B * J, n), device=dev, dtype=torch.float32)
    d.pred_out, d.anchors3d_out, d.anchors2d_out, d.valid_out, d.x_out, d.ol_out = _p(pred), _p(a3), _p(a2), _p(valid, torch.uint8), _p(x), _p(ol)
    _launch("egr_pose_query_f32", lib.egr_pose_query_f32, C.byref(d), _stream(), flops=2.0 * B * (Cdim * 3 * J + J * Cdim * (2 * Cdim + n + 4)))
    return pred, a3, a2, valid, x, ol



# --------------------------------------------------------------------------- launch-device record hygiene
def _guarded(fn):
    """A wrapper whose host-side validation raises after its first _p() must not leave the thread's launch-device record set."""
    import functools

    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except BaseException:
            _DEVL.idx = None
            raise
    return run


def _guard_module(ns):
    import types
    for _name, _fn in list(ns.items()):
        if isinstance(_fn, types.FunctionType) and not _name.startswith("_") and _fn.__module__ == ns.get("__name__"):
            ns[_name] = _guarded(_fn)


_guard_module(globals())
