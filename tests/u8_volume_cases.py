"""Byte volumes (rf_input_dtype RF_IO_U8, three dimensions): the shapes, filters and setups shared by
tests/test_u8_volumes_host.py and tests/test_gpu_u8_volumes.py (a plain module: no tests, no fixtures).  The per-sample rule,
the inputs (byte_image(shape, seed_of(shape))) and the f32 reference are those of tests/u8_cases.py, as they stand.

A byte volume is NATIVE where its depth is a multiple of 32, its width a multiple of 4 and it is filtered along z and along x
and / or y: the x/y result waits in an f32 volume of the plan's own and the final z pass stores the bytes."""
from __future__ import annotations

import numpy as np

import ref_cases as rc
from recfilter_amd import capi

TILED = capi.RF_PLAN_TILED_ONLY
FUSED, AUTO = capi.RF_PATH_TILED_FUSED, capi.RF_PATH_AUTO
IO = dict(dtype=np.float32, input_dtype=np.uint8, output_dtype=np.uint8)
IN = dict(dtype=np.float32, input_dtype=np.uint8)

# numpy order (z, y, x).  What each reaches of the final z pass (256 lines per workgroup, lines = x * y):
SHAPES = [
    (64, 128, 512),      # whole tiles, the uniform instances
    (64, 96, 128),       # a partial tile column in x/y, uniform
    (96, 200, 260),      # partial tiles both ways, lines no multiple of 256: the general instance; three z tiles of 32
    (32, 40, 260),       # one z tile
    (256, 64, 256),      # four z tiles of 64 (32 / 128 with RF_PLAN_TILE_PLANES)
]
GPU_SHAPES = SHAPES[:3]

Z_PATTERNS = ["pair", "causal", "anticausal"]


def scans_of(coeff, zpat):
    z = {"pair": [(2, True, coeff), (2, False, coeff)], "causal": [(2, True, coeff)], "anticausal": [(2, False, coeff)]}[zpat]
    return rc.xy_pm(coeff) + z


# (name, prologue, epilogue): no epilogue has an input operand (such a plan is staged)
SETUPS = [
    ("plain", None, None),
    ("round_trip", (1.0 / 255.0, 0.0), (255.0, 0.0, 0.0)),
    ("half_plus_16", None, (0.5, 0.0, 16.0)),
    ("negative", None, (-1.0, 0.0, 200.0)),
]
SETUP_IDS = [s[0] for s in SETUPS]

ORDER1 = [0.25, 0.75]          # a first-order low pass of unit gain
