"""egr_conv_aux.in_mode = EGR_IN_UP2_RELU (the operand ReLU(up2(x)) interpolated as the launch loads the half-resolution x): what the
host decides - the plan of the launches the streaming route covers, and EGR_EINVAL, from egr_conv_plan and from the launching entry
points alike, for everything else.  No GPU: raw C ABI with fake, aligned pointers (none is dereferenced on these paths, and a
refused call returns before anything is launched)."""
import ctypes as C

import pytest

from egorear_amd import hip

P = 0x10000          # 16-byte aligned fake device pointer


def _desc(**kw):
    """The lifting head's first conv at the smallest size the streaming route takes: 16 images, 1x1 128 -> 64 over the 64 x 64 image
    that the 32 x 32 source up-samples to."""
    d = hip.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout = 16, 64, 64, 128, 64
    d.kh = d.kw = d.stride = 1
    d.pad, d.ho, d.wo = 0, 64, 64
    d.ldx, d.ldy, d.ldr = 128, 64, 64
    d.xmap = hip.NMap(16, 32 * 32 * 128, 0)
    d.ymap = hip.NMap(16, 64 * 64 * 64, 0)
    d.rmap = hip.NMap(1, 0, 0)
    d.act, d.res_mode, d.split_k, d.groups, d.w_format = 1, 0, 1, 1, hip.W_F16X2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _aux(in_mode=hip.IN_UP2_RELU, up2_out=None, **kw):
    a = hip.ConvAux(P, P, None, None, None, 0, in_mode, up2_out)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _plan(d, aux, res=None, mask=None):
    pl = hip.ConvPlan()
    rc = hip.lib.egr_conv_plan(C.byref(d), P, P, None, None, res, None, None, mask, P, None, 0, C.byref(aux), C.byref(pl))
    return rc, pl


def _entry(d, aux, res=None):
    return hip.lib.egr_conv2d_nhwc_ex_f32(C.byref(d), P, P, None, None, res, None, None, P, None, 0, C.byref(aux), None)


def test_aux_struct_layout():
    """egr_conv_aux: six 8-byte members, then int32 in_mode (padded to 8) and the pointer in_up2_out."""
    assert C.sizeof(hip.ConvAux) == 64
    assert hip.ConvAux.in_mode.offset == 48 and hip.ConvAux.in_up2_out.offset == 56
    a = hip.ConvAux(P, P, None)                # the callers that name the first members only get the plain mode
    assert a.in_mode == hip.IN_PLAIN and a.in_up2_out is None


@pytest.mark.parametrize("cout,up2_out,variant", [(64, None, 1820), (128, None, 1840), (64, P, 2820), (128, P, 2840)])
def test_plan_reports_the_mode(cout, up2_out, variant):
    rc, pl = _plan(_desc(cout=cout, ldy=cout, ymap=hip.NMap(16, 64 * 64 * cout, 0)), _aux(up2_out=up2_out))
    assert rc == 0
    assert (pl.route, pl.variant, pl.planes, pl.bm, pl.bn) == (hip.ROUTE_STREAM_1X1, variant, 2, 32, cout)
    # the same launch without the mode: the same route, tile and grid
    rc0, p0 = _plan(_desc(cout=cout, ldy=cout, ymap=hip.NMap(16, 64 * 64 * cout, 0), xmap=hip.NMap(16, 64 * 64 * 128, 0)), _aux(hip.IN_PLAIN))
    assert rc0 == 0 and p0.variant == variant % 1000
    assert (p0.route, p0.grid_x, p0.grid_y, p0.grid_z, p0.block) == (pl.route, pl.grid_x, pl.grid_y, pl.grid_z, pl.block)


def test_grouped_and_non_square_plans():
    rc, pl = _plan(_desc(n=4, groups=4, gx=4 * 32 * 32 * 128, gw=64 * 128 * 2, gp=64, gy=4 * 64 * 64 * 64), _aux())
    assert rc == 0 and (pl.route, pl.variant, pl.grid_z) == (hip.ROUTE_STREAM_1X1, 1820, 4)
    rc, pl = _plan(_desc(h=32, w=128, ho=32, wo=128, xmap=hip.NMap(16, 16 * 64 * 128, 0)), _aux())       # 16 x 64 source
    assert rc == 0 and pl.variant == 1820


REFUSED = {
    "stride 2": dict(stride=2, ho=32, wo=32),
    "3x3 stride 2": dict(kh=3, kw=3, pad=1, stride=2, ho=32, wo=32, cout=256, ldy=256),
    "3x3 stride 1": dict(kh=3, kw=3, pad=1),
    "padded 1x1": dict(pad=1, ho=66, wo=66),
    "odd height": dict(h=63, ho=63),
    "odd width": dict(w=63, wo=63),
    "width not a multiple of 32": dict(w=80, wo=80),
    "output smaller than the image": dict(ho=32, wo=32),
    "bf16x3": dict(w_format=1),
    "fp32": dict(w_format=0),
    "transposed": dict(transposed=1),
    "out_nchw": dict(out_nchw=1),
    "cin 64": dict(cin=64, ldx=64),
    "GELU": dict(act=2),
    "split K": dict(split_k=2),
    "too few rows for the streaming route": dict(n=8),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_unsupported_calls_are_refused_by_plan_and_entry(why):
    d = _desc(**REFUSED[why])
    for aux in (_aux(), _aux(up2_out=P)):
        assert _plan(d, aux)[0] == hip.EINVAL, why
        assert _entry(d, aux) == hip.EINVAL, why


def test_side_operands_are_refused():
    d = _desc()
    assert _plan(d, _aux(in_mode=2))[0] == hip.EINVAL and _entry(d, _aux(in_mode=2)) == hip.EINVAL        # no such mode
    assert _plan(d, _aux(hip.IN_PLAIN, up2_out=P))[0] == hip.EINVAL                                       # an output without the mode
    assert _plan(d, _aux(up2_out=P + 4))[0] == hip.EINVAL and _entry(d, _aux(up2_out=P + 4)) == hip.EINVAL
    # residual, in both places
    r = _desc(res_mode=1)
    assert _plan(r, _aux(), res=P)[0] == hip.EINVAL and _entry(r, _aux(), res=P) == hip.EINVAL
    # training variants: the statistics epilogue (TR 1) and the masked data gradient (TR 2)
    tiles = C.c_int32(0)
    bn = _aux(bn_partials=P, bn_tiles_out=C.addressof(tiles), bn_capacity=1 << 30)
    s = _desc(act=0)
    assert _plan(s, bn)[0] == hip.EINVAL and _entry(s, bn) == hip.EINVAL
    assert _plan(s, _aux(), mask=P)[0] == hip.EINVAL
    assert hip.lib.egr_conv2d_masked_ex_f32(C.byref(s), P, P, None, P, P, None, 0, C.byref(_aux()), None) == hip.EINVAL
    # the operand written out must stay inside 32-bit byte offsets: 2^31 bytes per group and more are refused
    big = _desc(n=1024, xmap=hip.NMap(1024, 32 * 32 * 128, 0), ymap=hip.NMap(1024, 64 * 64 * 64, 0))
    assert _plan(big, _aux())[0] == 0 and _plan(big, _aux(up2_out=P))[0] == hip.EINVAL
    assert _plan(_desc(n=1023, xmap=hip.NMap(1023, 32 * 32 * 128, 0), ymap=hip.NMap(1023, 64 * 64 * 64, 0)), _aux(up2_out=P))[0] == 0


def test_chain_entry_refuses_the_mode():
    d = _desc(cout=128, ldy=128)
    ch = hip.ChainAux(P, P, None, 128, 1, 0, 0)
    assert hip.lib.egr_conv1x1_chain_f32(C.byref(d), P, P, None, None, P, C.byref(_aux()), C.byref(ch), None) == hip.EINVAL


def test_policy_field_and_its_switch():
    assert hip.LaunchPolicy().up2_on_load is True
    assert hip.LaunchPolicy.from_env({}).up2_on_load is True
    assert hip.LaunchPolicy.from_env({"EGR_UP2_ON_LOAD": "0"}).up2_on_load is False
    # not a pack-shaping field: packs made with it on serve with it off
    assert hip.LaunchPolicy().replace(up2_on_load=False).pack_key() == hip.LaunchPolicy().pack_key()
