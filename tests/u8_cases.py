"""Byte planes on both sides (rf_input_dtype RF_IO_U8): the cases, the inputs and the per-sample rule shared by
tests/test_u8_output_host.py and tests/test_gpu_u8_output.py (a plain module: no tests, no fixtures).

The contract: out = sat8(v), sat8(v) = (uint8) min(max(rint(v), 0), 255), v the f32 result behind the epilogue, converted once.

The one-rounding rule, per sample:   |got - clip(want, 0, 255)| <= 0.5 + delta,   delta = TOL * scale
  want   the f64 oracle of the widened bytes through the same pointwise stages (rc.pointwise_want)
  0.5    half a unit of the one rounding to an integer
  delta  the suite's f32 bar (TOL = 1e-4) applied to the magnitude of the terms the result is a sum of: the per-sample `scale`
         rc.pointwise_want returns for a plan with an epilogue, |want| for one without (a Gaussian of non-negative bytes keeps
         its sign: the strict pointwise relative error).  Derived from the number formats, not measured.  (Per sample it is never
         more than TOL times the image's peak, so this reading of the rule is the narrow one.)
A path that rounds an intermediate to bytes misses the rule by up to 0.5."""
from __future__ import annotations

import numpy as np

import ref_cases as rc
from recfilter_amd import capi

TOL = 1e-4
TILED = capi.RF_PLAN_TILED_ONLY

# (shape, flags beyond RF_PLAN_TILED_ONLY, what it covers): the smallest shapes at which the byte final pass can go wrong
NATIVE_SHAPES = [
    ((2 * 128 + 70, 5 * 256), capi.RF_PLAN_TILE_ROWS(128), "partial_rows_tall"),
    ((4 * 128, 2 * 256 + 4), capi.RF_PLAN_TILE_ROWS(128), "last_column_4_wide"),
    ((3 * 64 + 20, 3 * 256 + 8), capi.RF_PLAN_TILE_ROWS(64), "rows64"),
    ((5 * 32, 2 * 256), capi.RF_PLAN_TILE_ROWS(32), "rows32"),
]
NATIVE_IDS = [s[2] for s in NATIVE_SHAPES]

# (name, prologue, epilogue)
SETUPS = [
    ("plain", None, None),
    ("round_trip", (1.0 / 255.0, 0.0), (255.0, 0.0, 0.0)),
    ("unsharp", None, (-1.0, 2.0, 0.0)),          # leaves [0, 255] on both sides
]
SETUP_IDS = [s[0] for s in SETUPS]

# the Gaussian cases of the one-rounding rule: every native shape with GAUSS2, the first one with GAUSS3 as well
GAUSS_CASES = [(i, "GAUSS2") for i in range(len(NATIVE_SHAPES))] + [(0, "GAUSS3")]
GAUSS_IDS = [f"{NATIVE_IDS[i]}-{c}" for i, c in GAUSS_CASES]

STAGED_SHAPES = [((64, 250), rc.xy_pm(rc.GAUSS2), "odd_width"),
                 ((40, 16, 272), rc.REFERENCE_TESTS["test_generic_xyz"]["scans"], "volume")]


def seed_of(shape, plane=0):
    return 9000 + 131 * plane + sum(int(s) * (i + 1) for i, s in enumerate(shape)) % 997


def byte_image(shape, seed):
    """uniform random bytes, fixed seed"""
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


def sat8(v):
    """the contract's conversion, in numpy (np.rint rounds ties to even; NaN -> 0)"""
    v = np.asarray(v)
    return np.clip(np.rint(np.nan_to_num(v, nan=0.0)), 0, 255).astype(np.uint8)


def want_and_scale(img_u8, scans, clamped, prologue=None, epilogue=None):
    """(want, scale) of the rule for one byte plane"""
    want, scale = rc.pointwise_want(img_u8.astype(np.float32), scans, clamped, prologue, epilogue)
    if scale is None:
        scale = np.abs(want)
    return want, scale


def rule_excess(got_u8, want, scale):
    """max over samples of |got - clip(want, 0, 255)| - (0.5 + TOL * scale): the rule holds where this is <= 0"""
    d = np.abs(np.asarray(got_u8, dtype=np.float64) - np.clip(want, 0.0, 255.0))
    return float(np.max(d - (0.5 + TOL * np.asarray(scale, dtype=np.float64))))


def f32_reference_bytes(img_u8, scans, clamped, prologue=None, epilogue=None):
    """sat8 of the oracle run in f32 (as tests/metric_margin.py runs it) through the pointwise stages in f32: what a correct f32
    implementation with one conversion at the end produces"""
    import oracle
    x = img_u8.astype(np.float32)
    if prologue is not None:
        x = np.float32(prologue[0]) * x + np.float32(prologue[1])
    f = oracle.apply_filter(x, scans, clamped)
    assert f.dtype == np.float32
    if epilogue is not None:
        f = np.float32(epilogue[0]) * f + (np.float32(epilogue[1]) * x + np.float32(epilogue[2]))
    return sat8(f)
