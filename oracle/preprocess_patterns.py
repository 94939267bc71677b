"""Edge shapes and pixel patterns of the pre-processing tests.  TEST INFRASTRUCTURE ONLY.

One home for what oracle/make_golden_preprocess.py feeds to Pillow and what tests/test_preprocess.py and
tests/test_gpu_preprocess.py regenerate: the frames come from seeds (egorear_amd.synth's counter-based generator, the same
bytes under every numpy version), only Pillow's answers are stored (tests/golden/preprocess_pil_edges.npz).
"""
from __future__ import annotations

import functools

import numpy as np

from egorear_amd import synth
from oracle import preprocess_oracle as O

# (in_hw, out_hw) of the two-pass launches: every horizontal-pass kernel at its edges (tests/test_gpu_preprocess.py says which)
TWO_PASS_SHAPES = (
    ((36, 40), (48, 64)), ((200, 64), (40, 320)), ((88, 72), (16, 24)), ((100, 24), (20, 8)), ((48, 64), (48, 64)),
    ((35, 44), (24, 20)), ((35, 44), (40, 64)), ((36, 45), (24, 20)),
    ((33, 47), (24, 20)), ((64, 330), (16, 64)), ((96, 100), (20, 24)),
)
# (in_hw, out_hw) given to the one-launch kernel; the last one is just over its LDS limit and falls back to two passes
FUSED_SHAPES = (
    ((64, 128), (80, 256)), ((60, 64), (100, 256)), ((100, 512), (40, 256)), ((44, 256), (30, 256)), ((500, 400), (100, 256)),
    ((532, 400), (100, 256)), ((536, 400), (100, 256)),
)
# every launch refuses this one (its vertical window has 25 taps, one step over the accepted 23); Pillow and the oracle do not
HOST_ONLY_SHAPES = (((560, 400), (100, 256)),)
SHAPES = TWO_PASS_SHAPES + FUSED_SHAPES + HOST_ONLY_SHAPES
# one shape per kernel (LDS, aligned-dword, generic, fused) for the saturating patterns; the first, second and last up-sample
PATTERN_SHAPES = (((36, 40), (48, 64)), ((35, 44), (40, 64)), ((33, 47), (24, 20)), ((64, 128), (80, 256)))
PATTERNS = ("random", "zeros", "ones", "checker1", "blocks3", "blocks5", "binary")
FRAMES = 2                 # frames per case
FULL_BYTES = 32 * 1024     # a Pillow answer up to this size is stored whole, a larger one as every 4th pixel + its sum


def frame(pattern: str, h: int, w: int, seed: int) -> np.ndarray:
    """One (h, w, 3) uint8 frame of the named pattern."""
    if pattern == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if pattern == "ones":
        return np.full((h, w, 3), 255, np.uint8)
    if pattern in ("checker1", "blocks3", "blocks5"):
        b = {"checker1": 1, "blocks3": 3, "blocks5": 5}[pattern]
        y, x = np.mgrid[0:h, 0:w]
        on = ((y // b + x // b + seed) % 2).astype(bool)           # the seed flips the phase between the frames of a batch
        return np.repeat(np.where(on, 255, 0).astype(np.uint8)[:, :, None], 3, axis=2)
    u = synth.uniform01(f"preprocess.edges.{pattern}.{h}x{w}", seed, h * w * 3).reshape(h, w, 3)
    if pattern == "random":
        return (u * np.float32(256.0)).astype(np.uint8)            # 24 random bits: exact, 0 .. 255
    if pattern == "binary":
        return np.where(u < np.float32(0.5), 0, 255).astype(np.uint8)   # every channel of every pixel on its own
    raise ValueError(pattern)


def frames(pattern: str, in_hw, n: int = FRAMES, seed: int = 0) -> np.ndarray:
    """(n, h, w, 3) uint8: frames seed .. seed + n - 1 of the pattern."""
    return np.stack([frame(pattern, in_hw[0], in_hw[1], seed + i) for i in range(n)])


@functools.lru_cache(maxsize=None)
def oracle_u8(pattern: str, in_hw, out_hw, n: int = FRAMES, seed: int = 0) -> np.ndarray:
    """(n, oh, ow, 3) uint8: the numpy oracle's resized image of frames(pattern, in_hw, n, seed); computed once, read-only."""
    out = np.stack([O.pil_bicubic_resize_u8(f, out_hw[0], out_hw[1]) for f in frames(pattern, in_hw, n, seed)])
    out.flags.writeable = False
    return out


def cases():
    """Every (pattern, in_hw, out_hw) the golden file answers: random bytes at every shape, every pattern at PATTERN_SHAPES."""
    out = [("random", i, o) for i, o in SHAPES]
    out += [(p, i, o) for i, o in PATTERN_SHAPES for p in PATTERNS if p != "random"]
    return out


def key(pattern: str, in_hw, out_hw, i: int) -> str:
    return f"{pattern}_{in_hw[0]}x{in_hw[1]}_{out_hw[0]}x{out_hw[1]}_f{i}"


def golden_entries(k: str, out: np.ndarray) -> dict:
    """What the golden file keeps of one resized (oh, ow, 3) uint8 image."""
    if out.nbytes <= FULL_BYTES:
        return {k + "_full": np.ascontiguousarray(out)}
    return {k + "_sl": out[::4, ::4].copy(), k + "_sum": np.int64(out.astype(np.int64).sum())}


def check_against_golden(golden, k: str, out: np.ndarray) -> None:
    """Assert that `out` is the image the golden file holds under key k (whole, or every 4th pixel and the sum)."""
    if k + "_full" in golden.files:
        np.testing.assert_array_equal(out, golden[k + "_full"], err_msg=k)
    else:
        np.testing.assert_array_equal(out[::4, ::4], golden[k + "_sl"], err_msg=k)
        assert int(out.astype(np.int64).sum()) == int(golden[k + "_sum"]), k
