#!/usr/bin/env python3
"""Signature of the plans the builders produce, for comparing two builds of the library.

For a fixed list of filter descriptions (CASES) this builds every plan host-only (RF_DEVICE_HOST_ONLY: no GPU needed) and
writes one JSON record per plan: path, tiles, workspace_bytes, num_kernels, num_exchanges, the exchange sizes, has_interior
and, for every table the plan exposes through rf_plan_table, its length and the SHA-256 of its bytes.  A refactor of the
host-side plan builders must leave every record as it was (tables bit for bit):

    RECFILTER_AMD_LIB=/path/to/old/librecfilter_amd.so python tools/plan_signature.py > old.jsonl
    python tools/plan_signature.py > new.jsonl
    python tools/plan_signature.py --compare old.jsonl new.jsonl

--steps (needs a GPU): plans small enough to run are also built on the device and executed once with
rf_plan_execute_timed; the record then carries the step names in launch order.
--golden: only the integer fields (no hashes of floating-point tables, which may differ between toolchains) as ONE JSON
document -- what tests/golden/plan_signature.json holds and tests/test_plan_signature.py compares against.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recfilter_amd as rfa                      # noqa: E402
from recfilter_amd import capi                   # noqa: E402

X, Y, Z = 0, 1, 2
C, A = True, False
GAUSS2 = [0.0975842401, 1.5283848, -0.625968993]
GAUSS3 = [0.0226432718, 2.29634666, -1.79971004, 0.480720282]
_a = 2.0 - math.sqrt(3.0)
BICUBIC = [1.0 + _a, -_a]
SUM1 = [1.0, 1.0]
FILTERS = {"gauss2": GAUSS2, "gauss3": GAUSS3, "bicubic": BICUBIC, "sum1": SUM1}
ORDER5 = [0.01, 2.6, -2.9, 1.7, -0.52, 0.066]            # a stable order-5 low-pass (poles inside the unit circle)
ORDER9 = [1.0] + [0.05] * 9
CFG5 = [(X, C, [1.0, 0.5, 0.25]), (X, A, [1.0, 0.5, 0.125]), (Y, C, [1.0, 0.5, 0.0625]), (Y, A, [1.0, 0.5, 0.125]),
        (Z, C, [1.0, 0.5, 0.25]), (Z, A, [1.0, 0.5, 0.0625])]
FUSED, GENERIC, OVERLAP = capi.RF_PATH_TILED_FUSED, capi.RF_PATH_TILED_GENERIC, capi.RF_PATH_TILED_OVERLAPPED
TILED = capi.RF_PLAN_TILED_ONLY

TABLE_NAMES = (["scans", "seg_R_x", "seg_P_x", "neighbour_carries", "clamp1d_w", "clamp1d_G", "clamp1d_H", "clamp1d_L"]
               + [f"{p}_{d}" for p in ("W", "A", "G", "H", "prop", "X", "Y") for d in "xyz"]
               + [f"mx_{p}_{d}" for p in ("G", "R", "dG", "H", "dH", "A", "pair", "H21", "v21", "W21", "levels", "geom") for d in "xyz"])


def xy_pm(co):
    return [(X, C, list(co)), (X, A, list(co)), (Y, C, list(co)), (Y, A, list(co))]


def _cases():
    cases = []

    def add(name, shape, scans, **kw):
        cases.append((name, dict(shape=tuple(shape), scans=scans, **kw)))

    # ---- fused 2-D f32 -----------------------------------------------------------------------------------------------
    shapes2d = [(96, 512), (512, 1024), (512, 1028), (326, 1280), (2112, 2112), (4096, 4096), (5000, 5000), (16384, 16384),
                (16380, 16384)]
    for fname, co in FILTERS.items():
        for clamped in (True, False):
            b = "clamp" if clamped else "zero"
            for shp in shapes2d:
                for full in (0, capi.RF_PLAN_FULL_CARRY_SCAN):
                    add(f"fused2d_{fname}_{b}_{shp[0]}x{shp[1]}" + ("_fullscan" if full else ""), shp, xy_pm(co), clamped=clamped,
                        path=FUSED, flags=full)
            for full in (0, capi.RF_PLAN_FULL_CARRY_SCAN):
                add(f"fused2d_{fname}_{b}_1280sq_x3" + ("_fullscan" if full else ""), (1280, 1280), xy_pm(co), clamped=clamped,
                    planes=3, path=FUSED, flags=full)
    for rows in (32, 64, 128):
        for shp in [(512, 1024), (4096, 4096), (5000, 5000)]:
            add(f"fused2d_gauss2_rows{rows}_{shp[0]}x{shp[1]}", shp, xy_pm(GAUSS2), clamped=True, path=FUSED,
                flags=capi.RF_PLAN_TILE_ROWS(rows))
        add(f"fused2d_gauss3_rows{rows}_4096sq", (4096, 4096), xy_pm(GAUSS3), clamped=True, path=FUSED,
            flags=capi.RF_PLAN_TILE_ROWS(rows))
    add("fused2d_gauss2_1280sq_x3_nobatch", (1280, 1280), xy_pm(GAUSS2), clamped=True, planes=3, path=FUSED,
        flags=capi.RF_PLAN_NO_PLANE_BATCH)
    add("fused2d_gauss2_u8_2048sq", (2048, 2048), xy_pm(GAUSS2), clamped=True, path=FUSED, input_dtype=np.uint8,
        prologue=(1.0 / 255.0, 0.0))
    add("fused2d_gauss2_unsharp_4096sq", (4096, 4096), xy_pm(GAUSS2), clamped=True, path=FUSED, epilogue=(-0.5, 1.5, 0.0))
    add("fused2d_gauss3_unsharp_16384sq", (16384, 16384), xy_pm(GAUSS3), clamped=True, path=FUSED, epilogue=(-0.5, 1.5, 0.0))
    add("fused2d_gauss2_prologue_2048sq", (2048, 2048), xy_pm(GAUSS2), clamped=True, path=FUSED, prologue=(2.0, -0.5),
        epilogue=(1.0, 0.0, 0.25))
    add("fused2d_xonly_2048sq", (2048, 2048), xy_pm(GAUSS2)[:2], clamped=True, path=FUSED)
    add("fused2d_yonly_2048sq", (2048, 2048), xy_pm(GAUSS2)[2:], clamped=True, path=FUSED)
    add("fused2d_xonly_one_scan_4096sq", (4096, 4096), xy_pm(GAUSS2)[:1], clamped=False, path=FUSED)
    add("fused2d_yonly_one_scan_16384sq", (16384, 16384), xy_pm(GAUSS2)[2:3], clamped=False, path=FUSED)
    add("fused2d_auto_1024sq", (1024, 1024), xy_pm(GAUSS2), clamped=True)
    add("fused2d_auto_tiled_1024sq", (1024, 1024), xy_pm(GAUSS2), clamped=True, flags=TILED)
    add("fused2d_three_x_scans_2048sq", (2048, 2048), [(X, C, GAUSS2), (X, A, GAUSS2), (X, C, BICUBIC), (Y, C, GAUSS3)],
        clamped=True, path=FUSED)
    # ---- pixel types -------------------------------------------------------------------------------------------------
    for dt in ("float64", "int32", "int16", "float16", "bfloat16"):
        integer = dt.startswith("int")
        co = [1.0, 1.0] if integer else GAUSS2
        add(f"fused2d_{dt}_1024x2048", (1024, 2048), xy_pm(co) if not integer else [(X, C, co), (Y, C, co)],
            clamped=not integer, path=FUSED, dtype=dt)
        add(f"auto2d_{dt}_1024x2048", (1024, 2048), xy_pm(co) if not integer else [(X, C, co), (Y, C, co)],
            clamped=not integer, dtype=dt, flags=TILED)
    add("staged_f16_300x1001", (300, 1001), xy_pm(GAUSS2), clamped=True, dtype="float16", flags=TILED)
    add("staged_bf16_forced_1024x2048", (1024, 2048), xy_pm(GAUSS2), clamped=True, dtype="bfloat16",
        flags=TILED | capi.RF_PLAN_STAGE_HALF)
    # ---- 1-D chained rows --------------------------------------------------------------------------------------------
    biquad = [1.0, 1.2, -0.5]
    add("chain1d_2p20", (1 << 20,), [(X, C, biquad)], path=FUSED)
    add("chain1d_10M_inplace_tail", (10_000_000,), [(X, C, biquad)], path=FUSED)
    add("chain1d_10M_epilogue_padded", (10_000_000,), [(X, C, biquad)], path=FUSED, epilogue=(1.0, 0.5, 0.0))
    for n in (1, 2, 4):
        add(f"chain1d_8192x64_{n}scans", (8192 * 64,), [(X, C, biquad)] * n, path=FUSED)
    add("chain1d_2p24_order3_two_scans", (1 << 24,), [(X, C, GAUSS3), (X, A, GAUSS3)], path=FUSED)
    add("chain1d_pair_cascade_1000000", (1_000_000,), [(X, C, biquad), (X, A, biquad)], flags=TILED)
    add("chain1d_f16_2p20", (1 << 20,), [(X, C, biquad)], path=FUSED, dtype="float16")
    add("clamped1d_2p20", (1 << 20,), [(X, C, GAUSS2), (X, A, GAUSS2)], clamped=True, flags=TILED)
    add("clamped1d_100000", (100_000,), [(X, C, GAUSS3), (X, A, GAUSS3)], clamped=True, flags=TILED)
    # ---- clamped sections --------------------------------------------------------------------------------------------
    add("sections_order5_256x512", (256, 512), xy_pm(ORDER5), clamped=True, flags=TILED)
    add("sections_order5_2048sq", (2048, 2048), xy_pm(ORDER5), clamped=True, flags=TILED)
    add("sections_order5_zero_2048sq", (2048, 2048), xy_pm(ORDER5), clamped=False, flags=TILED)
    # ---- 3-D ---------------------------------------------------------------------------------------------------------
    for n in (256, 512, 1024, 2048):
        add(f"vol_cfg5_{n}cubed", (n, n, n), CFG5, path=FUSED)
    add("vol_cfg5_512cubed_staged", (512, 512, 512), CFG5, path=FUSED, flags=capi.RF_PLAN_STAGED_PASS1)
    add("vol_cfg5_256cubed_walk", (256, 256, 256), CFG5, path=FUSED, flags=capi.RF_PLAN_WALK_PASS1)
    add("vol_cfg5_1024x1021x1021_walk", (1024, 1021, 1021), CFG5, path=FUSED, flags=capi.RF_PLAN_WALK_PASS1)
    add("vol_cfg5_1024x1021x1021", (1024, 1021, 1021), CFG5, path=FUSED)
    add("vol_cfg5_2048cubed_inplace_z", (2048, 2048, 2048), CFG5, path=FUSED, flags=capi.RF_PLAN_INPLACE_Z)
    add("vol_cfg5_2048cubed_rows64", (2048, 2048, 2048), CFG5, path=FUSED, flags=capi.RF_PLAN_TILE_ROWS(64))
    add("vol_cfg5_clamped_512cubed", (512, 512, 512), CFG5, path=FUSED, clamped=True)
    add("vol_cfg5_epilogue_512cubed", (512, 512, 512), CFG5, path=FUSED, epilogue=(1.0, 0.5, 0.0))
    add("vol_gauss3_512cubed", (512, 512, 512), xy_pm(GAUSS3) + [(Z, C, GAUSS3), (Z, A, GAUSS3)], path=FUSED, clamped=True)
    add("vol_i32_256cubed", (256, 256, 256), [(X, C, SUM1), (Y, C, SUM1), (Z, C, SUM1)], path=FUSED, dtype="int32")
    add("vol_f64_128cubed", (128, 128, 128), CFG5, path=FUSED, dtype="float64")
    add("vol_generic_z_100x512x512", (100, 512, 512), CFG5, path=FUSED)
    add("vol_z_only_256cubed", (256, 256, 256), CFG5[4:], flags=TILED)
    add("vol_sections_order5_128x256x256", (128, 256, 256), xy_pm(ORDER5) + [(Z, C, GAUSS2)], clamped=True, flags=TILED)
    # ---- shards ------------------------------------------------------------------------------------------------------
    for world, ranks in ((2, (0, 1)), (8, (0, 3, 7))):
        for r in ranks:
            add(f"rows_w{world}_r{r}_gauss2", (4096 // world, 4096), xy_pm(GAUSS2), clamped=True, path=FUSED, shard_rank=r,
                shard_world=world)
    add("rows_w8_r3_gauss2_rows128", (1024, 4096), xy_pm(GAUSS2), clamped=True, path=FUSED, shard_rank=3, shard_world=8,
        flags=capi.RF_PLAN_TILE_ROWS(128))
    four_y3 = xy_pm(GAUSS3)[:2] + [(Y, C, GAUSS3), (Y, A, GAUSS3)] * 2
    for r in (0, 9, 15):
        add(f"rows_w16_r{r}_four_order3_y", (256, 2048), four_y3, clamped=True, path=FUSED, shard_rank=r, shard_world=16)
    for r in (0, 1, 2):
        add(f"rows_w3_unequal_r{r}", ((1024, 512, 2048)[r], 2048), xy_pm(GAUSS2), clamped=False, path=FUSED, shard_rank=r,
            shard_world=3, shard_extents=(1024, 512, 2048))
    add("rows_w2_r1_f64", (512, 1024), xy_pm(GAUSS2), clamped=True, path=FUSED, shard_rank=1, shard_world=2, dtype="float64")
    add("rows_w2_r0_x3_planes", (512, 1024), xy_pm(GAUSS2), clamped=True, path=FUSED, shard_rank=0, shard_world=2, planes=3)
    add("rows_force_exchange", (1024, 1024), xy_pm(GAUSS2), clamped=True, path=FUSED, flags=capi.RF_PLAN_FORCE_EXCHANGE)
    for r in (0, 3, 7):
        add(f"zslab_w8_r{r}_cfg5_early", (64, 512, 512), CFG5, path=FUSED, shard_rank=r, shard_world=8)
        add(f"zslab_w8_r{r}_cfg5_late", (64, 512, 512), CFG5, path=FUSED, shard_rank=r, shard_world=8,
            flags=capi.RF_PLAN_LATE_EXCHANGE)
    add("zslab_w8_r3_cfg5_walk_1024", (128, 1024, 1024), CFG5, path=FUSED, shard_rank=3, shard_world=8)
    add("zslab_w8_r3_cfg5_staged_1024", (128, 1024, 1024), CFG5, path=FUSED, shard_rank=3, shard_world=8,
        flags=capi.RF_PLAN_STAGED_PASS1)
    add("zslab_w2_r1_epilogue", (128, 512, 512), CFG5, path=FUSED, shard_rank=1, shard_world=2, epilogue=(1.0, 0.5, 0.0))
    four_z3 = CFG5[:4] + [(Z, C, GAUSS3), (Z, A, GAUSS3)] * 2
    add("zslab_w16_r5_four_order3_z", (64, 256, 256), four_z3, path=FUSED, shard_rank=5, shard_world=16)
    add("zslab_w2_unequal_r1", (192, 256, 256), CFG5, path=FUSED, shard_rank=1, shard_world=2, shard_extents=(64, 192))
    add("zslab_force_exchange", (128, 256, 256), CFG5, path=FUSED, flags=capi.RF_PLAN_FORCE_EXCHANGE)
    add("zslab_w4_r2_generic_z", (100, 256, 256), CFG5, path=FUSED, shard_rank=2, shard_world=4)
    # ---- generic path ------------------------------------------------------------------------------------------------
    add("generic_1d_tile32", (4096,), [(X, C, GAUSS2), (X, A, GAUSS2)], path=GENERIC, tile=(32,))
    add("generic_2d_tile16", (320, 480), xy_pm(GAUSS2), clamped=True, path=GENERIC, tile=(16, 16))
    add("generic_3d_tile8", (64, 64, 64), CFG5, path=GENERIC, tile=(8, 8, 8))
    add("generic_2d_f64", (320, 480), xy_pm(GAUSS3), clamped=True, path=GENERIC, tile=(32, 32), dtype="float64")
    add("generic_2d_i16", (320, 480), [(X, C, SUM1), (Y, C, SUM1)], path=GENERIC, tile=(32, 32), dtype="int16")
    add("generic_1d_order9_serial", (4096,), [(X, C, ORDER9)], path=GENERIC, tile=(64,))
    add("generic_2d_order9_w2_r1", (256, 512), [(X, C, ORDER9), (Y, C, ORDER9), (Y, A, ORDER9)], path=GENERIC, tile=(64, 64),
        shard_rank=1, shard_world=2)
    for r in (0, 1):
        add(f"generic_2d_w2_r{r}", (160, 480), xy_pm(GAUSS2), clamped=True, path=GENERIC, tile=(16, 16), shard_rank=r,
            shard_world=2)
    add("generic_2d_w16_r4_four_order3_y", (64, 512), four_y3, clamped=True, path=GENERIC, tile=(32, 32), shard_rank=4,
        shard_world=16)
    add("generic_3d_w4_r2", (16, 64, 64), CFG5, path=GENERIC, tile=(8, 8, 8), shard_rank=2, shard_world=4)
    add("generic_2d_x3_planes", (320, 480), xy_pm(GAUSS2), path=GENERIC, tile=(16, 16), planes=3)
    # ---- overlapped path ---------------------------------------------------------------------------------------------
    add("overlap_2d_tile32", (512, 512), xy_pm(GAUSS2), clamped=True, path=OVERLAP, tile=(32, 32))
    add("overlap_2d_xonly_scans", (512, 512), xy_pm(GAUSS3)[:3], clamped=False, path=OVERLAP, tile=(64, 16))
    add("overlap_3d_tile8", (64, 64, 64), CFG5, path=OVERLAP, tile=(8, 8, 8))
    add("overlap_3d_tile16_clamped_f64", (64, 64, 64), CFG5, clamped=True, path=OVERLAP, tile=(16, 16, 16), dtype="float64")
    add("overlap_2d_i32", (256, 256), [(X, C, SUM1), (Y, C, SUM1)], path=OVERLAP, tile=(32, 32), dtype="int32")
    # ---- the decisions of build_plan itself (plan.cpp): every stage, every wrapper, every refusal ------------------------
    bq, first = [0.05, 1.6, -0.7], [0.5, 0.5]
    NO_CASCADE, MATRIX, UNTILED = capi.RF_PLAN_NO_CASCADE, capi.RF_PATH_TILED_MATRIX, capi.RF_PATH_UNTILED
    # the in-plan cascade
    add("cascade1d_5_biquads_1000000", (1_000_000,), [(X, C, bq)] * 5, flags=TILED)
    add("cascade1d_9_biquads_1000000", (1_000_000,), [(X, C, bq)] * 9, flags=TILED)
    add("cascade1d_padded_pair_100000", (100_000,), [(X, C, bq), (X, A, bq)], flags=TILED)
    add("cascade2d_six_x_one_y_clamped", (256, 512), [(X, C, first)] * 6 + [(Y, A, [0.6, 0.4])], clamped=True, flags=TILED)
    add("cascade_refused_input_epilogue", (256, 512), [(X, C, first)] * 5, flags=TILED, epilogue=(1.0, 1.0, 0.0))
    add("cascade_off_1000000", (1_000_000,), [(X, C, bq)] * 5, flags=TILED | NO_CASCADE)
    add("cascade_off_forced_fused_refused", (1_000_000,), [(X, C, bq)] * 5, path=FUSED, flags=NO_CASCADE)
    add("cascade_forced_fused_64sq", (64, 64), [(X, C, first)] * 5, path=FUSED)
    add("cascade_forced_fused_stage_refused", (256, 512), [(X, C, ORDER9)] * 2, path=FUSED)
    # clamped 1-D signals
    add("clamped1d_over_cascade_100000", (100_000,), [(X, C, bq)] * 5, clamped=True, flags=TILED)
    add("clamped1d_running_sum_refused", (100_000,), [(X, C, SUM1)], clamped=True, flags=TILED)
    # merged runs
    r, th = 0.9995, 0.01
    slow = [1e-3, 2 * r * math.cos(th), -r * r]
    mild = [(X, C, [0.5, 0.3, 0.1]), (X, C, [0.8, 0.2]), (X, C, [0.7, 0.2, -0.1]), (X, A, [0.6, 0.3]), (X, A, [0.9, 0.1, 0.05]),
            (X, A, [0.6, 0.4])]
    add("merged_five_fast_2p20", (1 << 20,), [(X, C, [1.0, 0.1, 0.1])] * 5)
    add("merged_refused_slow_poles_2p20", (1 << 20,), [(X, C, slow)] * 2)
    add("merged_kept_as_given_2p20", (1 << 20,), mild)
    # the matrix path and the automatic choice
    add("matrix1d_order15_2p16", (1 << 16,), [(X, C, [1.0] + [0.01] * 15)])
    add("matrix1d_order5_one_scan_2p20", (1 << 20,), [(X, C, ORDER5)])
    add("matrix1d_order5_one_scan_clamped_2p20", (1 << 20,), [(X, C, ORDER5)], clamped=True)
    add("matrix2d_order9_y_96x160", (96, 160), [(Y, A, ORDER9)], clamped=True)
    add("matrix_forced_refused_100x162", (100, 162), [(X, A, ORDER9)], path=MATRIX)
    add("auto_order9_generic_100x162", (100, 162), [(X, A, ORDER9)])
    add("auto_order9_untiled_101x103", (101, 103), [(X, C, ORDER9)])
    add("auto_lines_512sq", (512, 512), xy_pm(GAUSS2), clamped=True)
    add("auto_lines_order3_1920sq", (1920, 1920), xy_pm(GAUSS3), clamped=True)
    add("auto_overlap_five_x_tile32", (512, 512), [(X, C, first)] * 5 + [(Y, C, first)], tile=(32, 32), flags=NO_CASCADE)
    add("untiled_serial_100sq", (100, 100), xy_pm(GAUSS2), path=UNTILED, flags=capi.RF_PLAN_SERIAL_UNTILED)
    add("untiled_no_scans_auto", (64, 64), [])
    add("untiled_no_scans_forced", (64, 64), [], path=UNTILED)
    add("untiled_1d_f64_10007", (10007,), [(X, C, GAUSS2)], dtype="float64")
    add("forced_overlap_refused_no_tiles", (512, 512), xy_pm(GAUSS2), path=OVERLAP)
    add("forced_fused_refused_f64_order9", (256, 512), [(X, C, ORDER9)], path=FUSED, dtype="float64")
    # 16-bit pixels: staged and native
    add("staged_f16_lines_1d_4099", (4099,), [(X, C, GAUSS2)], dtype="float16")
    add("staged_f16_two_planes_300x1001", (300, 1001), xy_pm(GAUSS2), clamped=True, dtype="float16", flags=TILED,
        epilogue=(-0.5, 1.5, 0.0))
    add("staged_f16_width_302", (100, 302), xy_pm(GAUSS2), clamped=True, dtype="float16")
    add("staged_bf16_over_cascade_1000000", (1_000_000,), [(X, C, bq)] * 5, dtype="bfloat16", flags=TILED)
    add("staged_f16_over_generic_256x512", (256, 512), [(Y, C, first)] * 5, dtype="float16", flags=TILED, epilogue=(1.0, 1.0, 0.0))
    add("staged_f16_vol_64x96x128", (64, 96, 128), CFG5, dtype="float16")
    add("native_f16_vol_forced_64x96x128", (64, 96, 128), CFG5, dtype="float16", path=FUSED)
    add("native_f16_vol_128x256x256", (128, 256, 256), CFG5, dtype="float16")
    add("staged_f16_vol_fused_builder_refused", (100, 256, 256), CFG5, dtype="float16", path=FUSED)
    add("staged_f16_vol_sharded_refused", (128, 256, 256), CFG5, dtype="float16", shard_rank=0, shard_world=2)
    # clamped sections
    add("sections_order5_256x512_x3", (256, 512), xy_pm(ORDER5), clamped=True, flags=TILED, planes=3)
    add("sections_off_zero_2048sq", (2048, 2048), xy_pm(ORDER5), clamped=False, flags=TILED | capi.RF_PLAN_NO_SECTIONS)
    # stand-alone pointwise steps
    add("pointwise_generic_f64", (320, 480), xy_pm(GAUSS2), clamped=True, path=GENERIC, tile=(32, 32), dtype="float64",
        prologue=(2.0, -0.5), epilogue=(1.0, 0.5, 0.25))
    add("pointwise_generic_u8", (320, 480), xy_pm(GAUSS2), clamped=True, path=GENERIC, tile=(32, 32), input_dtype=np.uint8,
        prologue=(1.0 / 255.0, 0.0), epilogue=(1.0, 0.5, 0.0))
    # refusals of the validation
    add("refused_tile_not_a_divisor", (100, 100), xy_pm(GAUSS2), tile=(32, 32))
    add("refused_unknown_path", (64, 64), xy_pm(GAUSS2), path=9)
    add("refused_stream_and_staged_pass1", (512, 512), xy_pm(GAUSS2), path=FUSED,
        flags=capi.RF_PLAN_STREAM_PASS1 | capi.RF_PLAN_STAGED_PASS1)
    return cases


CASES = _cases()


def _dtype(name):
    if name == "bfloat16":
        import torch
        return torch.bfloat16
    return np.dtype(name)


def _plan(kw, device):
    kw = dict(kw)
    kw["dtype"] = _dtype(kw.get("dtype", "float32"))
    kw.setdefault("flags", 0)           # (not recfilter_amd.plan.DEFAULT_FLAGS, which the test suite changes)
    return rfa.Plan(device=device, **kw)


def _tables(plan, with_hash):
    L = capi.lib()
    out = {}
    for name in TABLE_NAMES:
        n = ctypes.c_size_t()
        if L.rf_plan_table(plan._h, name.encode(), None, 0, ctypes.byref(n)) != capi.RF_OK:
            continue
        rec = {"len": int(n.value)}
        if with_hash:
            rec["sha256"] = hashlib.sha256(np.ascontiguousarray(plan.table(name)).tobytes()).hexdigest()
        out[name] = rec
    return out


def signature(kw, with_hash=True):
    """The record of one description (host-only)."""
    try:
        plan = _plan(kw, capi.RF_DEVICE_HOST_ONLY)
    except rfa.capi.RecFilterError as e:
        return {"status": e.status, "error": str(e)} if with_hash else {"status": e.status}
    with plan:
        rec = {"status": 0, "path": plan.path_name, "tiles": list(plan.tiles), "workspace_bytes": plan.workspace_bytes,
               "num_kernels": plan.num_kernels, "num_exchanges": plan.num_exchanges,
               "exchange_bytes": [plan.exchange_bytes(i) for i in range(plan.num_exchanges)],
               "has_interior": bool(plan.has_interior), "tables": _tables(plan, with_hash)}
        if "neighbour_carries" in rec["tables"]:
            _, tx, _, ty = plan.table("neighbour_carries")
            rec["neighbour_form"] = [bool(tx), bool(ty)]
    return rec


def step_names(kw, max_bytes):
    """Step names of one execute on the GPU (unsharded plans whose planes fit `max_bytes`); None where not run."""
    import torch
    if kw.get("shard_world", 1) > 1 or kw.get("flags", 0) & capi.RF_PLAN_FORCE_EXCHANGE:
        return None                  # (a sharded plan is driven through the stepping calls)
    dt = _dtype(kw.get("dtype", "float32"))
    item = 2 if dt is not None and str(dt).endswith("float16") else np.dtype(dt).itemsize
    planes = kw.get("planes", 1)
    if int(np.prod(kw["shape"])) * item * planes * 2 > max_bytes:
        return None
    try:
        plan = _plan(kw, -1)
    except rfa.capi.RecFilterError as e:
        return f"not built: {e}"
    with plan:
        tdt = rfa.plan._torch_dtype(plan.dtype_code)
        in_dt = torch.uint8 if plan.input_np_dtype is not None else tdt
        ins = [torch.zeros(kw["shape"], dtype=in_dt, device="cuda:0") for _ in range(planes)]
        outs = [torch.empty(kw["shape"], dtype=tdt, device="cuda:0") for _ in range(planes)]
        _, timed = plan.execute_timed(ins, outs)
        torch.cuda.synchronize()
        return [n for n, _ in timed]


def golden_record(kw):
    """The integer fields of one description; tables as {name: length}."""
    rec = signature(kw, with_hash=False)
    if "tables" in rec:
        rec["tables"] = {name: t["len"] for name, t in rec["tables"].items()}
    return rec


def golden_document():
    return {name: golden_record(kw) for name, kw in CASES}


def compare(old_path, new_path):
    """One line per case (workspace_bytes of both, a digest of the rest of both records), then the differences between two
    outputs of this tool, one line each; returns their number.  One difference is permitted and
    reported apart: workspace_bytes lower by a multiple of 16 up to 128 (rf_plan::alloc turns an empty upload into a 16-byte
    placeholder, and a builder may stop making some)."""
    old = {r["case"]: r for r in map(json.loads, open(old_path))}
    new = {r["case"]: r for r in map(json.loads, open(new_path))}
    bad, placeholders = 0, {}

    def digest(rec):         # of everything but workspace_bytes, which is printed beside it
        rest = {k: v for k, v in rec.items() if k != "workspace_bytes"}
        return hashlib.sha256(json.dumps(rest, sort_keys=True).encode()).hexdigest()[:16]
    for case in sorted(set(old) | set(new)):
        a, b = old.get(case), new.get(case)
        if a is not None and b is not None:
            print(f"{case} workspace_bytes {a.get('workspace_bytes')} {b.get('workspace_bytes')} record {digest(a)} {digest(b)}")
        if a is None or b is None:
            print(f"{case}: only in {'the first' if b is None else 'the second'} file")
            bad += 1
            continue
        for key in sorted(set(a) | set(b)):
            if a.get(key) == b.get(key):
                continue
            if key == "workspace_bytes":
                less = a[key] - b[key]
                if 0 < less <= 128 and less % 16 == 0:
                    placeholders[less] = placeholders.get(less, 0) + 1
                    continue
            if key == "tables":
                for name in sorted(set(a[key]) | set(b[key])):
                    if a[key].get(name) != b[key].get(name):
                        print(f"{case}: table {name}: {a[key].get(name)} -> {b[key].get(name)}")
                        bad += 1
                continue
            print(f"{case}: {key}: {a.get(key)} -> {b.get(key)}")
            bad += 1
    for less, count in sorted(placeholders.items()):
        print(f"permitted: workspace_bytes lower by {less} (placeholders of empty uploads) in {count} plans")
    print(f"{len(old)} / {len(new)} records, {bad} differences")
    return bad


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", action="store_true", help="also execute the plans that fit on the GPU and record their step names")
    ap.add_argument("--max-bytes", type=int, default=1 << 30, help="--steps: largest in + out footprint of a plan that is run")
    ap.add_argument("--golden", action="store_true", help="integer fields only, one JSON document")
    ap.add_argument("--only", default="", help="substring of the case names to run")
    args = ap.parse_args()
    if args.golden:
        json.dump(golden_document(), sys.stdout, sort_keys=True, separators=(",", ":"))
        print()
        return
    for name, kw in CASES:
        if args.only and args.only not in name:
            continue
        rec = {"case": name}
        rec.update(signature(kw))
        if args.steps:
            rec["steps"] = step_names(kw, args.max_bytes)
        print(json.dumps(rec, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
