"""Every path stays inside its planes and keeps no state across steps (tests/guarded.py has the checks).

One table, ROWS: a row is one plan description plus what proves it reaches the instance it is meant for (path, tiles, launch
names).  Every row runs

  1. one execute (rf_plan_execute_timed, for the launch names) on guarded planes: output guards unchanged, the input allocation
     bit-unchanged, the result through the suite's oracle assertion (floats: any NaN from the 0xFF input guards fails it;
     integer and uint8 planes: bit-identical between a 0xFF-guard and a 0x00-guard run);
  2. three_steps: A, poison (all NaN; another random image for integers), A on one plan and one stream -- step 3 bit-identical
     to step 1, one instance;
  3. poisoned_scratch: a new plan whose scratch buffers are all filled with 0xFF before its first execute -- bit-identical.

Shapes are the smallest that reach the instance; the largest is 2^22 samples.  The f64 oracle of a case is computed once and
shared by the rows that use it.  tests/test_footprint_host.py builds every row as a host-only plan and checks path and tiles
there, so a row that drifts off its instance shows without a GPU."""
import numpy as np
import pytest

import guarded
import ref_cases as rc
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

TILED = capi.RF_PLAN_TILED_ONLY
AUTO, UNTILED, GENERIC, FUSED, OVERLAP, MATRIX = (capi.RF_PATH_AUTO, capi.RF_PATH_UNTILED, capi.RF_PATH_TILED_GENERIC,
                                                  capi.RF_PATH_TILED_FUSED, capi.RF_PATH_TILED_OVERLAPPED, capi.RF_PATH_TILED_MATRIX)
ROWS_T = capi.RF_PLAN_TILE_ROWS
MAX_SAMPLES = 1 << 22

NP_OF = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i16": np.int16}


def _plan_dtype(kind):
    import torch
    return {"f16": torch.float16, "bf16": torch.bfloat16}.get(kind) or NP_OF[kind]


# ---- coefficient sets ------------------------------------------------------------------------------------------------------
XYZ = rc.REFERENCE_TESTS["test_generic_xyz"]["scans"]
G3 = rc.GAUSS3
XY_ORDER3 = [(0, True, G3), (0, False, G3), (1, True, G3), (1, False, G3)] + XYZ[4:]
_INT_COEFF = {1: [1.0, 1.0], 2: [1.0, 2.0, -1.0], 3: [1.0, 3.0, -3.0, 1.0]}       # integral images of order 1..3: ring arithmetic


def int_scans(scans):
    """the same dimensions, directions and orders with integer weights"""
    return [(d, c, _INT_COEFF[len(w) - 1]) for d, c, w in scans]


def stable_coeff(order, seed, b=0.4, mass=0.85):
    """tests/test_gpu_high_order.py: [b, a1..a_order] with sum |a| = mass < 1"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(order) * np.exp(-0.15 * np.arange(order))
    a *= mass / np.abs(a).sum()
    return [b] + [float(np.float32(v)) for v in a]


def audio_coeff(order):
    return [1.0] + [0.01] * order


def _from_poles(poles, b=0.3):
    p = np.poly(poles).real
    return [b] + [float(-v) for v in p[1:]]


ORDER5 = _from_poles([0.8, 0.5 + 0.3j, 0.5 - 0.3j, -0.2 + 0.6j, -0.2 - 0.6j], b=0.25)
ORDER5_POSITIVE = [0.5, 0.1, 0.1, 0.1, 0.1, 0.1]


def clamped_1d_scans(pattern, n):
    """tests/test_gpu_parity.py::test_clamped_1d_signals_on_the_fused_kernels: random stable scans, 'c' causal / 'a' anticausal"""
    rng = np.random.default_rng(len(pattern) * 1000 + n % 997)
    scans = []
    for ch in pattern:
        k = int(rng.integers(1, 4))
        co = [float(rng.uniform(0.3, 1.2))] + [float(-c) for c in np.poly(rng.uniform(-0.85, 0.85, size=k))[1:]]
        scans.append((0, ch == "c", co))
    return scans


# ---- the table -------------------------------------------------------------------------------------------------------------
ROWS = {}


def row(name, shape, scans, kind="f32", clamped=False, planes=1, path=FUSED, flags=TILED, tile=None, prologue=None, epilogue=None,
        u8=False, inplace=False, lead_in=0, lead_out=0, stepping=False, seed=500, group="", expect_path=None, expect_tiles=None,
        has=(), lacks=(), first=None):
    """expect_tiles: {dimension: tile}; has / lacks: substrings of launch names that must / must not occur; first: the first
    launch's name.  group: the path x type cell the row counts for (SUMMARY)."""
    assert name not in ROWS, name
    assert int(np.prod(shape)) <= MAX_SAMPLES, name
    ROWS[name] = dict(name=name, shape=tuple(shape), scans=list(scans), kind=kind, clamped=clamped, planes=planes, path=path, flags=flags,
                      tile=tile, prologue=prologue, epilogue=epilogue, u8=u8, inplace=inplace, lead_in=lead_in, lead_out=lead_out,
                      stepping=stepping, seed=seed, group=group or f"fused/{kind}", expect_path=FUSED if expect_path is None else expect_path,
                      expect_tiles=expect_tiles or {}, has=tuple(has), lacks=tuple(lacks), first=first)


# fused 2-D, f32: every FUSED_CASES shape out of place and in place
for _n, _c in rc.FUSED_CASES.items():
    for _ip in (False, True):
        row(f"fused2d-{_n}-{'inplace' if _ip else 'oop'}", _c["shape"], _c["scans"], clamped=_c["clamped"], inplace=_ip,
            has=("fused_pass2",), group="fused 2-D/f32")

# ... a subset in f64, int32 and int16 at widths that are multiples of 4
for _n in ("gauss2_clamped", "partial_gauss3_clamped", "partial_w4_gauss2_clamped", "partial_xy_gauss3_clamped", "partial_w4_mixed_zero"):
    _c = rc.FUSED_CASES[_n]
    row(f"fused2d-f64-{_n}", _c["shape"], _c["scans"], "f64", clamped=_c["clamped"], has=("fused_pass2",), group="fused 2-D/f64")
    for _k in ("i32", "i16"):
        row(f"fused2d-{_k}-{_n}", _c["shape"], int_scans(_c["scans"]), _k, clamped=_c["clamped"], inplace=(_k == "i16"),
            has=("fused_pass2",), group=f"fused 2-D/{_k}")

# tile heights (64 and 128 rows: the tall-tile instances), the full carry scans, both other first passes
_TALL = (2 * 128 + 70, 2 * 256 + 8)
for _r in (32, 64, 128):
    row(f"fused2d-tile_rows{_r}", _TALL, rc.xy_pm(rc.GAUSS2), clamped=True, flags=TILED | ROWS_T(_r), expect_tiles={0: 256, 1: _r},
        group="fused 2-D/f32")
    row(f"fused2d-tile_rows{_r}-order3-zero-inplace", _TALL, rc.xy_pm(G3), clamped=False, flags=TILED | ROWS_T(_r), inplace=True,
        expect_tiles={0: 256, 1: _r}, group="fused 2-D/f32")
row("fused2d-full_carry_scan", _TALL, rc.xy_pm(rc.GAUSS2), clamped=True, flags=TILED | ROWS_T(128) | capi.RF_PLAN_FULL_CARRY_SCAN,
    expect_tiles={1: 128}, has=("carry_y",), group="fused 2-D/f32")
row("fused2d-full_carry_scan-rows32", _TALL, rc.xy_pm(G3), clamped=True, flags=TILED | ROWS_T(32) | capi.RF_PLAN_FULL_CARRY_SCAN,
    expect_tiles={1: 32}, has=("carry_y",), group="fused 2-D/f32")
row("fused2d-mfma_pass1", _TALL, rc.xy_pm(rc.GAUSS2), clamped=True, flags=TILED | ROWS_T(128) | capi.RF_PLAN_MFMA_PASS1,
    expect_tiles={1: 128}, has=("fused_tails",), group="fused 2-D/f32")
row("fused2d-staged_pass1", _TALL, rc.xy_pm(rc.GAUSS2), clamped=True, flags=TILED | ROWS_T(128) | capi.RF_PLAN_STAGED_PASS1,
    expect_tiles={1: 128}, has=("fused_tails",), group="fused 2-D/f32")

# 3 and 5 planes, batched and one launch per plane
for _p in (3, 5):
    for _nb in (False, True):
        row(f"fused2d-planes{_p}-{'per_plane' if _nb else 'batched'}", (100, 528), rc.xy_pm(rc.GAUSS2), clamped=True, planes=_p,
            flags=TILED | (capi.RF_PLAN_NO_PLANE_BATCH if _nb else 0), inplace=(_p == 5), group="fused 2-D/f32")

# a last tile row shorter than the order: 1, 2, 65 and 130 rows (65 and 130 also on the tile heights that leave 1 and 2 rows)
for _h, _r in ((1, 0), (2, 0), (65, 0), (65, 64), (130, 0), (130, 128)):
    row(f"fused2d-rows{_h}-tile{_r or 'auto'}", (_h, 272), rc.xy_pm(G3), clamped=True, flags=TILED | (ROWS_T(_r) if _r else 0),
        expect_tiles={1: _r} if _r else None, group="fused 2-D/f32")

# f16 / bf16, native 2-D
for _k in ("f16", "bf16"):
    row(f"half2d-{_k}-rows128-partial_rows", (2 * 128 + 70, 5 * 256), rc.xy_pm(rc.GAUSS2), _k, clamped=True, flags=TILED | ROWS_T(128),
        expect_tiles={0: 256, 1: 128}, lacks=("convert",), group=f"fused 2-D native/{_k}")
    row(f"half2d-{_k}-rows128-wide_partial_column", (2 * 128, 24 * 256 + 4), rc.xy_pm(G3), _k, clamped=False, flags=TILED | ROWS_T(128),
        expect_tiles={0: 256, 1: 128}, lacks=("convert",), inplace=True, group=f"fused 2-D native/{_k}")
    row(f"half2d-{_k}-rows64", (3 * 64 + 20, 3 * 256 + 8), rc.xy_pm(rc.GAUSS2), _k, clamped=True, flags=TILED | ROWS_T(64),
        expect_tiles={1: 64}, lacks=("convert",), group=f"fused 2-D native/{_k}")
    row(f"half2d-{_k}-rows32", (5 * 32, 2 * 256), rc.xy_pm(rc.GAUSS2), _k, clamped=False, flags=TILED | ROWS_T(32),
        expect_tiles={1: 32}, lacks=("convert",), group=f"fused 2-D native/{_k}")
    row(f"half2d-{_k}-rows32-partial", (5 * 32 + 7, 2 * 256 + 12), rc.xy_pm(G3), _k, clamped=True, flags=TILED | ROWS_T(32),
        expect_tiles={1: 32}, lacks=("convert",), group=f"fused 2-D native/{_k}")
    # native volumes: the shapes of tests/test_gpu_half_volumes.py (the partial-general one 64 deep instead of 96: 2^22 samples at
    # most; its x/y extents, which choose the instances, are kept)
    _zp = [(2, True, rc.GAUSS2), (2, False, rc.GAUSS2)]
    for _n, _s in (("whole_uni", (64, 128, 512)), ("partial_uni", (64, 96, 128)), ("partial_general", (64, 200, 260))):
        row(f"halfvol-{_k}-{_n}-z_pair", _s, rc.xy_pm(rc.GAUSS2) + _zp, _k, clamped=True, lacks=("convert",), has=("strided_pass2_z",),
            inplace=(_n == "partial_uni"), group=f"fused 3-D native/{_k}")
    row(f"halfvol-{_k}-partial_general-z_causal", (64, 200, 260), rc.xy_pm(rc.GAUSS2) + _zp[:1], _k, clamped=True, lacks=("convert",),
        has=("strided_pass2_z",), group=f"fused 3-D native/{_k}")
    row(f"halfvol-{_k}-partial_general-z_anticausal", (64, 200, 260), rc.xy_pm(rc.GAUSS2) + _zp[1:], _k, clamped=False, lacks=("convert",),
        has=("strided_pass2_z",), group=f"fused 3-D native/{_k}")
    row(f"halfvol-{_k}-whole_uni-z_causal", (64, 128, 512), rc.xy_pm(rc.GAUSS2) + _zp[:1], _k, clamped=True, lacks=("convert",),
        has=("strided_pass2_z",), group=f"fused 3-D native/{_k}")
    # the staged forms: convert_in -> the f32 plan -> convert_out
    row(f"halfstaged-{_k}-odd_width", (300, 1001), rc.xy_pm(rc.GAUSS2), _k, clamped=True, path=AUTO, first="convert_in", has=("convert_out",),
        group=f"staged/{_k}")
    row(f"halfstaged-{_k}-order5_clamped", (256, 512), rc.xy_pm(ORDER5_POSITIVE), _k, clamped=True, path=AUTO, first="convert_in",
        has=("convert_out",), group=f"staged/{_k}")
    row(f"halfstaged-{_k}-small_volume_auto", (64, 96, 128), rc.xy_pm(rc.GAUSS2) + _zp, _k, clamped=True, path=AUTO, first="convert_in",
        has=("convert_out",), inplace=True, group=f"staged/{_k}")
    row(f"halfstaged-{_k}-stage_half_flag", (2 * 128, 3 * 256), rc.xy_pm(rc.GAUSS2), _k, clamped=True, planes=2, path=AUTO,
        flags=TILED | capi.RF_PLAN_STAGE_HALF, first="convert_in", has=("convert_out",), group=f"staged/{_k}")
    row(f"half1d-{_k}-100003", (100003,), [(0, True, rc.GAUSS2)], _k, lacks=("convert",), group=f"fused 1-D native/{_k}")

# uint8 input planes (the plans of test_uint8_input_planes), the input planes shifted by four bytes
_U8 = {"fused": ((128, 512), AUTO, FUSED), "fused_partial": ((75, 464), AUTO, FUSED), "generic_auto": ((64, 250), AUTO, None),
       "untiled": ((64, 256), UNTILED, UNTILED), "fused_3d": ((40, 16, 272), AUTO, FUSED)}
for _n, (_s, _p, _e) in _U8.items():
    for _post in (None, (-1.0, 2.0, 0.1)):
        row(f"u8-{_n}-{'unsharp' if _post else 'plain'}", _s, rc.xy_pm(rc.GAUSS2) if len(_s) == 2 else XYZ, clamped=len(_s) == 2, planes=2,
            path=_p, u8=True, prologue=(1.0 / 255.0, 0.0), epilogue=_post, lead_in=4, expect_path=-1 if _e is None else _e,
            group="uint8 input/f32")

# 3-D f32
row("vol-walk-two_tile_columns", (64, 96, 512), XYZ, clamped=True, flags=capi.RF_PLAN_WALK_PASS1, has=("walk_tails", "carry_planes_xy"),
    lacks=("strided_pass1_z",), group="fused 3-D/f32")
row("vol-walk-partial_tiles-order3-inplace", (64, 33, 260), XY_ORDER3, clamped=True, flags=capi.RF_PLAN_WALK_PASS1, has=("walk_tails",),
    inplace=True, group="fused 3-D/f32")
row("vol-walk-odd_width-tall", (32, 129, 387), XYZ, clamped=False, flags=capi.RF_PLAN_WALK_PASS1 | ROWS_T(128), has=("walk_tails",),
    expect_tiles={1: 128}, group="fused 3-D/f32")
# the strided z stage on 32-plane tiles (a depth that is no multiple of the 64 it prefers), order 3 along x and y
row("vol-strided_z-depth96-order3", (96, 40, 260), XY_ORDER3, clamped=True, flags=TILED | capi.RF_PLAN_STAGED_PASS1,
    has=("strided_pass1_z", "strided_pass2_z"), lacks=("walk_tails",), expect_tiles={2: 32}, group="fused 3-D/f32")
row("vol-strided_z-depth160-inplace", (160, 40, 132), XY_ORDER3, clamped=False, flags=TILED | capi.RF_PLAN_STAGED_PASS1,
    has=("strided_pass1_z",), expect_tiles={2: 32}, inplace=True, group="fused 3-D/f32")
# a depth no strided tile divides: the z stage runs on the generic passes behind the fused x/y stage
row("vol-generic_z-depth40-order3", (40, 96, 260), XY_ORDER3, clamped=True, flags=TILED | capi.RF_PLAN_STAGED_PASS1,
    has=("fused_pass2", "generic_pass1_z", "generic_pass2_z"), lacks=("strided_",), expect_tiles={2: 40}, group="fused 3-D/f32")
row("vol-generic_z-depth72-inplace", (72, 40, 132), XY_ORDER3, clamped=False, flags=TILED | capi.RF_PLAN_STAGED_PASS1,
    has=("generic_pass1_z",), lacks=("strided_",), inplace=True, group="fused 3-D/f32")
row("vol-three_planes-prologue", (64, 96, 128), XYZ, clamped=True, planes=3, prologue=(0.5, 0.25), has=("strided_pass2_z",),
    group="fused 3-D/f32")

# 1-D
for _n in (12345, 8192 * 3 + 2):
    row(f"sig-f32-{_n}", (_n,), [(0, True, rc.GAUSS2), (0, True, [0.7, 0.3])], lacks=("pad_copy",), group="fused 1-D/f32")
    for _pat in ("c", "ca", "ccccc"):
        row(f"sig-clamped-{_pat}-{_n}", (_n,), clamped_1d_scans(_pat, _n), clamped=True, path=AUTO, has=("clamp1d_dots", "clamp1d_fix"),
            inplace=(_pat == "ca"), group="fused 1-D clamped/f32")
    for _k in ("i32", "i16"):
        row(f"sig-{_k}-{_n}", (_n,), [(0, True, [1.0, 1.0]), (0, True, [2.0, -1.0, 1.0])], _k, group=f"fused 1-D/{_k}")

# line-parallel untiled (kernels_lines.hip), the four types; a volume
for _k in ("f32", "f64", "i32", "i16"):
    _sc = rc.xy_pm(G3) if _k[0] == "f" else [(0, True, [1.0, 2.0, -1.0]), (0, False, [1.0, 1.0]), (1, True, [1.0, 1.0]), (1, False, [2.0, 1.0, -1.0, 1.0])]
    row(f"lines-{_k}", (192, 320), _sc, _k, clamped=True, planes=2, path=UNTILED, expect_path=UNTILED, has=("line_scans_x", "line_scans_y"),
        inplace=(_k in ("f64", "i16")), group=f"line-parallel untiled/{_k}")
row("lines-f32-volume", (48, 32, 80), rc.xy_pm(G3) + [(2, True, rc.GAUSS2), (2, False, [0.5, 0.5])], clamped=True, path=UNTILED,
    expect_path=UNTILED, has=("line_scans_z",), group="line-parallel untiled/f32")
# one thread per line (a width that is no multiple of 16), planes shifted by one element
row("serial-untiled-200x250", (200, 250), rc.xy_pm(G3), clamped=True, path=UNTILED, expect_path=UNTILED, has=("untiled_scan_",),
    lead_in=1, lead_out=1, group="thread-per-line untiled/f32")
row("serial-untiled-200x250-inplace", (200, 250), rc.xy_pm(rc.GAUSS2), clamped=False, path=UNTILED, expect_path=UNTILED, has=("untiled_scan_",),
    lead_out=1, inplace=True, group="thread-per-line untiled/f32")

# generic tiled and overlapped tiled: the reference's own tests, literal tiles, planes shifted by one element
for _n, _c in rc.REFERENCE_TESTS.items():
    _t = [_c["tile"] if any(s[0] == d for s in _c["scans"]) else 0 for d in range(len(_c["shape"]))]
    _k = {np.float32: "f32", np.int16: "i16"}[_c["dtype"]]
    row(f"generic-{_n}", _c["shape"], _c["scans"], _k, clamped=_c["clamped"], path=GENERIC, tile=_t, expect_path=GENERIC,
        expect_tiles=dict(enumerate(_t)), has=("generic_pass1_",), lead_in=1, lead_out=1, group=f"generic tiled/{_k}")
    row(f"overlap-{_n}", _c["shape"], _c["scans"], _k, clamped=_c["clamped"], path=OVERLAP, tile=_t, expect_path=OVERLAP,
        expect_tiles=dict(enumerate(_t)), has=("overlap_pass1", "overlap_pass2"), lead_in=1, lead_out=1, inplace=(_n == "test_generic_xy"),
        group=f"overlapped tiled/{_k}")

# the matrix path, orders 12 and 29
for _o in (12, 29):
    row(f"matrix-1d-order{_o}", (1 << 16,), [(0, True, audio_coeff(_o)), (0, False, stable_coeff(_o, _o))], clamped=(_o == 29), path=MATRIX,
        expect_path=MATRIX, has=("mx_pass1_", "mx_pass2_"), seed=77, group="matrix/f32")
    _cf = stable_coeff(_o, 3)
    row(f"matrix-2d-order{_o}", (96, 160), [(0, True, _cf), (0, False, _cf), (1, True, _cf), (1, False, _cf)], clamped=(_o == 12), planes=2,
        path=MATRIX, expect_path=MATRIX, has=("mx_pass1_", "mx_pass2_"), seed=77, inplace=(_o == 29), group="matrix/f32")

# sections of order 5 behind the border modification: the caller's input must come back bit-unchanged (the form is "the
# zero-border scan of a modified input" -- the modification must never be made in the input planes)
_PM5 = rc.xy_pm(ORDER5)
row("sections-order5-clamped-one_tile", (128, 256), _PM5, clamped=True, path=AUTO, group="fused sections/f32")
row("sections-order5-clamped-many_tiles", (320, 1024), _PM5, clamped=True, path=AUTO, group="fused sections/f32")
row("sections-order5-clamped-narrow", (96, 48), _PM5, clamped=True, path=AUTO, group="fused sections/f32")
row("sections-order5-clamped-inplace", (320, 1024), _PM5, clamped=True, path=AUTO, inplace=True, group="fused sections/f32")

# in-plan cascades (tests/test_gpu_parity.py, _CASCADE_CASES)
_BIQUAD = [0.05, 1.6, -0.7]
row("cascade-six_x_rgb_partial_tiles", (250, 500), [(0, True, [0.5, 0.5])] * 6 + [(1, False, [0.6, 0.4])], clamped=True, planes=3, path=AUTO,
    has=("stage1.",), group="in-plan cascade/f32")
row("cascade-mixed_causality_padded_1d", (100_000,), [(0, True, _BIQUAD), (0, False, _BIQUAD)], path=AUTO, has=("stage1.",),
    group="in-plan cascade/f32")
row("cascade-five_x_int32", (300, 1024), [(0, True, [1.0, 1.0])] * 5 + [(1, True, [1.0, 1.0])], "i32", path=AUTO, has=("stage1.",),
    group="in-plan cascade/i32")
row("cascade-five_x_two_z_volume", (64, 96, 512), [(0, True, [0.5, 0.5])] * 5 + [(2, True, [0.6, 0.4])] * 2, path=AUTO, has=("stage1.",),
    inplace=True, group="in-plan cascade/f32")

# one rank driven through the stepping calls with the exchange structure
row("exchange-one_rank-stepping", (4 * 64, 3 * 256), rc.xy_pm(rc.GAUSS2), clamped=True, flags=TILED | capi.RF_PLAN_FORCE_EXCHANGE,
    stepping=True, group="fused 2-D exchange/f32")
row("exchange-one_rank-stepping-volume", (64, 72, 300), XYZ, clamped=True, flags=TILED | capi.RF_PLAN_FORCE_EXCHANGE, stepping=True,
    group="fused 3-D exchange/f32")


# ---- inputs, references ----------------------------------------------------------------------------------------------------
def inputs_of(r, seed_offset=0):
    """the row's input planes, host tensors of the input type"""
    import torch
    out = []
    for p in range(r["planes"]):
        seed = r["seed"] + seed_offset + p
        if r["u8"]:
            out.append(torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=r["shape"], dtype=np.uint8)))
        elif r["kind"] in ("f16", "bf16"):
            out.append(torch.from_numpy(rc.random_image(r["shape"], np.float32, seed)).to(_plan_dtype(r["kind"])))
        elif r["kind"] == "f64":
            out.append(torch.from_numpy(np.random.default_rng(seed).random(size=r["shape"])))
        else:
            out.append(torch.from_numpy(rc.random_image(r["shape"], NP_OF[r["kind"]], seed)))
    return out


def poison_of(r, A):
    if r["u8"] or r["kind"] in ("i32", "i16"):
        return inputs_of(r, seed_offset=7919)
    return [guarded.nan_like(t) for t in A]


_WANT = {}


def want_of(r, A):
    """[(want, scale)] per plane: the f64 oracle (bit-exact integer oracle) of the row's input, computed once per case"""
    import oracle
    key = (r["shape"], repr(r["scans"]), r["clamped"], r["kind"], r["u8"], r["planes"], r["seed"], r["prologue"], r["epilogue"])
    if key not in _WANT:
        res = []
        for t in A:
            if r["kind"] in ("i32", "i16"):
                res.append((oracle.apply_filter(t.numpy(), r["scans"], r["clamped"]), None))
            elif r["u8"]:
                x = np.float32(r["prologue"][0]) * t.numpy().astype(np.float32) + np.float32(r["prologue"][1])
                res.append(rc.pointwise_want(x, r["scans"], r["clamped"], None, r["epilogue"]))
            elif r["prologue"] or r["epilogue"]:
                res.append(rc.pointwise_want(t.numpy(), r["scans"], r["clamped"], r["prologue"], r["epilogue"]))
            else:
                wide = t.float().numpy().astype(np.float64) if r["kind"] in ("f16", "bf16") else t.numpy().astype(np.float64)
                res.append((oracle.apply_filter(wide, r["scans"], r["clamped"]), None))
        _WANT[key] = res
    return _WANT[key]


def make_plan(r, **kw):
    import recfilter_amd as rfa
    return rfa.Plan(r["shape"], r["scans"], dtype=_plan_dtype(r["kind"]), clamped=r["clamped"], planes=r["planes"], tile=r["tile"],
                    path=r["path"], flags=r["flags"], prologue=r["prologue"], epilogue=r["epilogue"],
                    input_dtype=np.uint8 if r["u8"] else None, **kw)


def check_instance(r, plan):
    """the plan is the one the row is meant for: path and tiles (host-only plans answer this too)"""
    if r["expect_path"] >= 0:
        assert plan.path == r["expect_path"], (r["name"], plan.path_name)
    for d, t in r["expect_tiles"].items():
        assert plan.tiles[d] == t, (r["name"], plan.tiles)


def check_names(r, names):
    for s in r["has"]:
        assert any(s in n for n in names), (r["name"], s, names)
    for s in r["lacks"]:
        assert not any(s in n for n in names), (r["name"], s, names)
    if r["first"]:
        assert names[0] == r["first"], (r["name"], names)


class _Stepping:
    """rf_plan_begin .. rf_plan_finish on one rank: the all-gather of one rank is the identity.  The send buffers are guarded
    allocations of their own, checked by done()."""

    def __init__(self, plan):
        self.plan, self.sends, self.names = plan, [], []

    def __call__(self, ins, outs):
        plan = self.plan
        assert plan.num_exchanges >= 1
        plan.begin(ins, outs)
        for i in range(plan.num_exchanges):
            views, g = guarded.guarded_planes((plan.exchange_bytes(i),), np.uint8, 1)
            views[0].zero_()
            self.sends.append(g)
            plan.exchange_local(i, views[0].data_ptr())
            plan.exchange_apply(i, views[0].data_ptr())
        plan.finish()

    def done(self):
        import torch
        torch.cuda.synchronize()
        for g in self.sends:
            g.check_guards("exchange send buffer")
        self.sends = []


class _Timed:
    def __init__(self, plan):
        self.plan, self.names = plan, []

    def __call__(self, ins, outs):
        _, timed = self.plan.execute_timed(ins, outs)
        self.names = [n for n, _ in timed]

    def done(self):
        pass


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a device that reports an error after a test is left alone: the session ends instead of starting more work on it"""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # pragma: no cover
        pytest.exit(f"the GPU reports an error after this test, nothing more is started on it: {e}", returncode=3)


@pytest.mark.parametrize("name", list(ROWS))
def test_footprint(name):
    import torch
    r = ROWS[name]
    A = inputs_of(r)
    poison = poison_of(r, A)
    wants = want_of(r, A)
    in_dt = torch.uint8 if r["u8"] else _plan_dtype(r["kind"])
    out_dt = _plan_dtype(r["kind"])
    integer = r["u8"] or r["kind"] in ("i32", "i16")
    with make_plan(r) as plan:
        check_instance(r, plan)
        first = _Stepping(plan) if r["stepping"] else _Timed(plan)
        got = guarded.guarded_execute(first, r["shape"], in_dt, out_dt, A, inplace=r["inplace"], in_fill=guarded.IN_FILL,
                                      lead_in=r["lead_in"], lead_out=r["lead_out"])
        first.done()
        if not r["stepping"]:
            check_names(r, first.names)
        for g, (want, scale) in zip(got, wants):
            err = guarded.assert_oracle(g, want, r["kind"], scale=scale)
        print(f"{name}: path {plan.path_name} tiles {plan.tiles} rel err {err:.3e}")
        if integer:
            again = guarded.guarded_execute(first, r["shape"], in_dt, out_dt, A, inplace=r["inplace"], in_fill=guarded.IN_FILL_ZERO,
                                            lead_in=r["lead_in"], lead_out=r["lead_out"])
            first.done()
            guarded.assert_bits_equal(again, got, "0x00 input guards against 0xFF input guards")
        step = _Stepping(plan) if r["stepping"] else None
        r1 = guarded.three_steps(plan, A, poison, out_dtype=out_dt, inplace=r["inplace"], execute=step)
        if step:
            step.done()
    with make_plan(r) as fresh:
        step = _Stepping(fresh) if r["stepping"] else None
        filled = guarded.poisoned_scratch(fresh, A, r1, out_dtype=out_dt, inplace=r["inplace"], execute=step)
        if step:
            step.done()
        kinds = [k for _, k, _ in fresh.debug_buffers()]
        print(f"{name}: {filled} scratch buffers filled of {len(kinds)} ({kinds.count('zeroed')} zeroed, {kinds.count('table')} tables)")


def test_cascade_that_runs_as_a_chain():
    """A front-end cascade with merge_cascades off: one plan per stage, stage 1 reads what stage 0 wrote.  The stages' plans
    run by hand on three guarded allocations (input, the stage boundary, output): every guard unchanged, the input and -- under
    stage 1 -- the boundary planes bit-unchanged, the result against the oracle on all eight scans; then three steps of the chain."""
    import torch
    import recfilter_amd as rfa
    shape = (96, 288)
    img = torch.from_numpy(rc.random_image(shape, np.float32, 21))
    x, y = rfa.RecFilterDim("x", shape[1]), rfa.RecFilterDim("y", shape[0])
    F = rfa.RecFilter("Chain")
    F.set_clamped_image_border()
    F[x, y] = img.cuda()
    for i in range(4):
        F.add_filter(+x if i % 2 == 0 else -x, [0.6, 0.3, 0.1])
        F.add_filter(+y if i % 2 == 0 else -y, [0.7, 0.3])
    scans = list(F._contents["scans"])
    rfa.RecFilter.merge_cascades = False
    try:
        stages = F.cascade([0, 1, 2, 3], [4, 5, 6, 7])
        for f in stages:
            f.split_all_dimensions(32)
        plans = [f.plan() for f in stages]
        assert all(f._contents["merged_stages"] == 0 for f in stages)
        assert [p.path for p in plans] == [FUSED, FUSED]

        def chain(ins, outs):
            mids, gm = guarded.guarded_planes(shape, np.float32, 1)
            plans[0].execute(ins, mids)
            torch.cuda.synchronize()
            gm.snapshot()
            plans[1].execute(mids, outs)
            torch.cuda.synchronize()
            gm.check_unchanged("stage boundary")
        got = guarded.guarded_execute(chain, shape, np.float32, np.float32, [img])
        import oracle
        guarded.assert_oracle(got[0], oracle.apply_filter(img.numpy().astype(np.float64), scans, True), "f32")

        class Both:
            num_instances = 1

        def two(ins, outs):
            plans[0].execute(ins, outs)
            plans[1].execute(outs, outs)
        guarded.three_steps(Both, [img], [guarded.nan_like(img)], execute=two)
        assert plans[0].num_instances == 1 and plans[1].num_instances == 1
    finally:
        rfa.RecFilter.merge_cascades = True


def test_debug_fill_refuses_tables_and_bad_indices():
    import recfilter_amd as rfa
    with rfa.Plan((128, 512), rc.xy_pm(rc.GAUSS2), clamped=True, path=FUSED) as plan:
        bufs = plan.debug_buffers()
        kinds = {k for _, k, _ in bufs}
        assert kinds == {"table", "zeroed", "scratch"}, kinds
        assert sum(b for _, _, b in bufs) == plan.workspace_bytes
        table = next(i for i, k, _ in bufs if k == "table")
        with pytest.raises(rfa.capi.RecFilterError) as e:
            plan.debug_fill(table, 0xFF)
        assert e.value.status == capi.RF_ERR_INVALID_ARG
        with pytest.raises(rfa.capi.RecFilterError):
            plan.debug_fill(len(bufs), 0)
        with pytest.raises(rfa.capi.RecFilterError):
            plan.debug_fill(-1, 0)
