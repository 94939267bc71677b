"""egorear_amd.run_reference: the reference's run.py on a PRISTINE checkout (VERDICT r4 missing #2 / next #6a).  The checkout is a
stand-in written by the `checkout` fixture with the layout the launcher relies on: run.py at the top, `pose_estimation` and
`pose_estimation.models` as namespace packages, an estimator package that must never execute (it raises when imported) and a
deformable-attention module that imports mmcv's MSDA Function.  Every check runs in a child interpreter so that the sys.modules /
sys.path / cwd changes of install() do not leak into the test session."""
import os
import subprocess
import sys
import textwrap

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STANDIN = {
    "run.py": '''
        """Stand-in entry point: reports that it ran, in which process, with which arguments and which estimator module."""
        import os
        import sys

        import pose_estimation.models.estimator as E

        print("RUN", __name__, os.getpid(), os.getcwd(), sys.argv[1:], E.__egorear_amd__)
    ''',
    "pose_estimation/models/estimator/__init__.py": '''
        raise ImportError("the checkout's own estimator package was executed")
    ''',
    "pose_estimation/models/estimator/egoposeformer_mvf_ex.py": '''
        raise ImportError("the checkout's own estimator files were executed")
    ''',
    "pose_estimation/models/utils/deform_attn.py": '''
        """Multi-scale deformable attention (Deformable DETR form) around mmcv's op."""
        import torch
        import torch.nn.functional as F
        from mmcv.ops.multi_scale_deform_attn import MultiScaleDeformableAttnFunction
        from torch import nn


        class MSDeformAttn(nn.Module):
            def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
                super().__init__()
                self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
                self.im2col_step = 64
                self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
                self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
                self.value_proj = nn.Linear(d_model, d_model)
                self.output_proj = nn.Linear(d_model, d_model)

            def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index):
                n, lq, _ = query.shape
                h, l, p = self.n_heads, self.n_levels, self.n_points
                value = self.value_proj(input_flatten).view(n, input_flatten.shape[1], h, self.d_model // h)
                off = self.sampling_offsets(query).view(n, lq, h, l, p, 2)
                aw = F.softmax(self.attention_weights(query).view(n, lq, h, l * p), -1).view(n, lq, h, l, p)
                normalizer = torch.stack([input_spatial_shapes[..., 1], input_spatial_shapes[..., 0]], -1)
                loc = reference_points[:, :, None, :, None, :] + off / normalizer[None, None, None, :, None, :]
                out = MultiScaleDeformableAttnFunction.apply(value, input_spatial_shapes, input_level_start_index, loc, aw, self.im2col_step)
                return self.output_proj(out)
    ''',
}


@pytest.fixture(scope="module")
def checkout(tmp_path_factory):
    root = tmp_path_factory.mktemp("egorear_checkout")
    for rel, text in STANDIN.items():
        path = root / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(textwrap.dedent(text).lstrip())
    return str(root)


def _run(args, code=None):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-c", code] if code is not None else [sys.executable, "-m", "egorear_amd.run_reference"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=REPO)


def test_check_mode_lists_the_three_classes_and_the_op(checkout):
    r = _run([checkout, "--check"])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    for name in ("EgoPoseFormerHeatmap", "EgoPoseFormerHeatmapMVFEX", "EgoPoseFormerMVFEX"):
        assert f"pose_estimation.models.estimator.{name} -> egorear_amd.estimator.{name}" in lines
    assert any(l.startswith("mmcv.ops.multi_scale_deform_attn.MultiScaleDeformableAttnFunction -> egorear_amd.msda.") for l in lines)


def test_reference_imports_bind_to_this_package_without_touching_the_gpu_or_the_references_estimator_files(checkout):
    code = f"""
import sys, os, torch
def ck(c, msg=""):
    if not c:
        raise SystemExit("FAILED: " + str(msg))
from egorear_amd import run_reference, estimator, msda
run_reference.install({checkout!r})
ck(os.getcwd() == {checkout!r} and sys.path[0] == {checkout!r})
# the wrappers' own import statements (pl_wrappers/egoposeformer/heatmap.py:21, heatmap_mvf_ex.py:23, pose_3d_mvf_ex.py:20)
from pose_estimation.models.estimator import EgoPoseFormerHeatmap
from pose_estimation.models.estimator import EgoPoseFormerHeatmapMVFEX
from pose_estimation.models.estimator import EgoPoseFormerMVFEX
import pose_estimation.models.estimator as E
ck(EgoPoseFormerHeatmap is estimator.EgoPoseFormerHeatmap and EgoPoseFormerHeatmapMVFEX is estimator.EgoPoseFormerHeatmapMVFEX)
ck(EgoPoseFormerMVFEX is estimator.EgoPoseFormerMVFEX and E.__egorear_amd__)
ck(not any(k.startswith("pose_estimation.models.estimator.") for k in sys.modules), [k for k in sys.modules if "estimator" in k])
# the checkout's own deformable-attention module, imported from the checkout, now calls this package's op
from pose_estimation.models.utils import deform_attn
ck(deform_attn.__file__.startswith({checkout!r}))
ck(deform_attn.MultiScaleDeformableAttnFunction is msda.MultiScaleDeformableAttnFunction)
m = deform_attn.MSDeformAttn(d_model=64, n_levels=1, n_heads=4, n_points=4).to("meta")
shapes = torch.tensor([[8, 8]], device="meta"); starts = torch.tensor([0], device="meta")
q, ref, tok = torch.empty(2, 5, 64, device="meta"), torch.empty(2, 5, 1, 2, device="meta"), torch.empty(2, 64, 64, device="meta")
out = m(q, ref, tok, shapes, starts)
ck(out.shape == (2, 5, 64), out.shape)           # the module's forward ran end to end on the op's Meta kernel
# (that the same statement sequence traces as ONE Dynamo graph with the operator in it: tests/test_msda_op_host.py)
ck(not torch.cuda.is_initialized())
# a YAML's model block constructs through the reference-path name
from egorear_amd import configs
net = EgoPoseFormerMVFEX(**configs.pose3d_cfg("ego4view_syn"))
ck(type(net).__module__ == "egorear_amd.estimator" and len(net.state_dict()) == 698)
print("OK")
"""
    r = _run(None, code)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_install_refuses_when_the_references_estimator_is_already_imported(checkout):
    code = f"""
import sys, types
sys.modules["pose_estimation.models.estimator"] = types.ModuleType("pose_estimation.models.estimator")
from egorear_amd import run_reference
try:
    run_reference.install({checkout!r})
except RuntimeError as e:
    assert "already imported" in str(e); print("OK")
"""
    r = _run(None, code)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_run_py_is_executed_in_process(checkout):
    """`fit|test ...` hands over to the checkout's run.py through runpy: same process (no exec), as `__main__`, in the checkout,
    with run.py's command line, and the estimator classes already bound to this package."""
    code = f"""
import os
from egorear_amd import run_reference
print("PID", os.getpid())
run_reference.main([{checkout!r}, "test", "--config", "configs/ego4view_syn_pose3d.yaml"])
"""
    r = _run(None, code)
    assert r.returncode == 0, r.stderr[-2000:]
    pid = [l.split()[1] for l in r.stdout.splitlines() if l.startswith("PID ")]
    run = [l for l in r.stdout.splitlines() if l.startswith("RUN ")]
    assert pid and run == [f"RUN __main__ {pid[0]} {checkout} ['test', '--config', 'configs/ego4view_syn_pose3d.yaml'] True"], r.stdout


def test_not_a_checkout_is_refused(tmp_path):
    r = _run([str(tmp_path), "--check"])
    assert r.returncode != 0 and "not an EgoRear checkout" in r.stderr
