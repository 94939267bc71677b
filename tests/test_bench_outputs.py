"""bench.py's --dump-outputs / --full options without a GPU: what the dump writes for the benchmarked shapes (every pose set in full,
each heat-map set as a fixed seeded sample, float32, within 64 MB) and that a plain run leaves the other legs off."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _forward_outputs(B):
    """Stand-ins of the forward's (list of 3-D pose sets, [initial, refined] heat maps) at batch B; every value is its flat index
    (exact in float32 below 2^24), so that a sample can be checked against the indices it claims."""
    preds = [torch.arange(B * 15 * 3, dtype=torch.float32).reshape(B, 15, 3) + k for k in range(4)]
    hms = [torch.arange(B * 4 * 15 * 64 * 64, dtype=torch.float32).reshape(B, 4, 15, 64, 64) for _ in range(2)]
    return preds, hms


def test_dump_at_the_benchmarked_batch(tmp_path):
    preds, hms = _forward_outputs(64)
    written = bench.dump_outputs((preds, hms), str(tmp_path / "a"))
    assert sorted(written) == [f"pred_heatmap_{i}" for i in range(2)] + [f"pred_pose3d_{i}" for i in range(4)]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in written)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for i, p in enumerate(preds):
        a = np.load(tmp_path / "a" / f"pred_pose3d_{i}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, p.numpy())
    idx = torch.randint(0, hms[0].numel(), (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).numpy()
    for i in range(2):
        a = np.load(tmp_path / "a" / f"pred_heatmap_{i}.npy")
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,)
        assert np.array_equal(a, idx.astype(np.float32))                  # the values at the seeded flat indices, in draw order
    bench.dump_outputs((preds, hms), str(tmp_path / "b"))                  # the same sample in every run
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_small_outputs_are_dumped_whole(tmp_path):
    preds, hms = _forward_outputs(2)
    bench.dump_outputs((preds, [h.double() for h in hms]), str(tmp_path))
    for i in range(2):
        a = np.load(tmp_path / f"pred_heatmap_{i}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, hms[i].numpy())


def test_plain_run_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs == ""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"
