"""The three launches on camera.packed_rays() records - triangulation, volumetric fusion, consensus - validate their cameras alike
(no GPU): one table of bad `cams` / `coord_trans_mat` / view counts / dtypes is refused by all three validators with ValueError, and
with dense=False, as the operators and their fake implementations call them, a valid operand need not be contiguous.  Meta tensors
throughout: a validator looks at shapes, dtypes and strides only."""
import pytest
import torch

B, J, K = 2, 3, 2


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def operands(V=4, batch=B):
    return {"coords": _meta(batch, V, J, 2), "conf": _meta(batch, V, J), "hm": _meta(batch, V, J, 8, 6), "centers": _meta(batch, J, 3),
            "cand": _meta(batch, V, J, K, 2), "cscore": _meta(batch, V, J, K), "cindex": _meta(batch, V, J, K, dtype=torch.int32),
            "cams": _meta(V, 30), "ctm": _meta(batch, V, 4, 4)}


def validate(which, o, dense):
    """-> (B, V) as the validator reports them"""
    from egorear_amd import hip
    if which == "triangulate":
        out = hip._tri_operands(o["coords"], o["conf"], o["cams"], o["ctm"], 1 / 64, 1 / 64, 1e-6, "test", dense=dense)
    elif which == "volume":
        out = hip._volume_operands(o["hm"], o["conf"], o["centers"], o["cams"], o["ctm"], None, 4, 40.0, 100.0, "test", dense=dense)
    else:
        out = hip._consensus_operands(o["cand"], o["cscore"], o["cindex"], o["cams"], o["ctm"], 1 / 64, 1 / 64, 2.0, 2, 1e-6, "test",
                                      dense=dense)
    return tuple(out[:2])


VALIDATORS = ("triangulate", "volume", "consensus")
MAIN = {"triangulate": "coords", "volume": "hm", "consensus": "cand"}
BAD = {
    "the shipped 17-float record": lambda w: dict(operands(), cams=_meta(4, 17)),
    "a record one float too long": lambda w: dict(operands(), cams=_meta(4, 31)),
    "three records for four views": lambda w: dict(operands(), cams=_meta(3, 30)),
    "one flat record": lambda w: dict(operands(), cams=_meta(120)),
    "one view": lambda w: operands(V=1),
    "five views": lambda w: operands(V=5),
    "coord_trans_mat of another batch": lambda w: dict(operands(), ctm=_meta(B + 1, 4, 4, 4)),
    "coord_trans_mat of three views": lambda w: dict(operands(), ctm=_meta(B, 3, 4, 4)),
    "coord_trans_mat 3 x 4": lambda w: dict(operands(), ctm=_meta(B, 4, 3, 4)),
    "coord_trans_mat without its batch": lambda w: dict(operands(), ctm=_meta(4, 4, 4)),
    "float64 records": lambda w: dict(operands(), cams=_meta(4, 30, dtype=torch.float64)),
    "float16 records": lambda w: dict(operands(), cams=_meta(4, 30, dtype=torch.float16)),
    "float64 coord_trans_mat": lambda w: dict(operands(), ctm=_meta(B, 4, 4, 4, dtype=torch.float64)),
    "float64 points or maps": lambda w: {k: (_meta(*v.shape, dtype=torch.float64) if k == MAIN[w] else v) for k, v in operands().items()},
}


@pytest.mark.parametrize("which", VALIDATORS)
@pytest.mark.parametrize("bad", sorted(BAD))
def test_every_validator_refuses_the_same_bad_cameras(which, bad):
    for dense in (True, False):
        with pytest.raises(ValueError):
            validate(which, BAD[bad](which), dense)


@pytest.mark.parametrize("which", VALIDATORS)
def test_a_valid_operand_need_not_be_contiguous_before_the_operator_makes_it_so(which):
    for V in (2, 3, 4):
        assert validate(which, operands(V), True) == (B, V)
        assert validate(which, dict(operands(V), ctm=None), True) == (B, V)
        for name, strided in (("cams", _meta(30, V).t()), ("ctm", _meta(B, V, 4, 4).transpose(-1, -2)),
                              (MAIN[which], operands(V)[MAIN[which]].transpose(0, 2).contiguous().transpose(0, 2))):
            o = dict(operands(V), **{name: strided})
            assert not strided.is_contiguous() and strided.shape == operands(V)[name].shape
            assert validate(which, o, False) == (B, V)
            with pytest.raises(ValueError):                  # a launch reads its operands as they lie
                validate(which, o, True)
