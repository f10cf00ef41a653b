"""Neighbour-form carries on the GPU: where a filter decays within a tile the fused x/y path completes a dimension's carries
from the neighbouring tiles' tails (plan_fused.cpp, neighbour_carry_bound) -- xscan_rows_kernel NB along x, the 128-row final
pass along y (FusedArgs::y_nb_W) -- and runs no carry_x / carry_y launch.  RF_PLAN_FULL_CARRY_SCAN keeps the scans: both forms
must agree to the last bits an f32 result shows, and both must pass the f64 oracle."""
import os

import numpy as np
import pytest

import oracle
import ref_cases as rc
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

TILED = capi.RF_PLAN_TILED_ONLY
FULL = capi.RF_PLAN_FULL_CARRY_SCAN
FUSED = capi.RF_PATH_TILED_FUSED


def _strict(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6)))


def _run(shape, scans, clamped, imgs, flags, inplace=False):
    import torch
    import recfilter_amd as rfa
    with rfa.Plan(shape, scans, clamped=clamped, planes=len(imgs), path=FUSED, flags=flags) as plan:
        dev = [torch.from_numpy(im).cuda() for im in imgs]
        if inplace:
            _, timed = plan.execute_timed(dev, dev)
            outs = dev
        else:
            outs, timed = plan.execute_timed(dev)
        got = [o.cpu().numpy() for o in outs]
        _, tx, _, ty = plan.table("neighbour_carries")
        tiles = plan.tiles
    return got, [n for n, _ in timed], (bool(tx), bool(ty)), tiles


@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3", "BICUBIC_COEFF"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("shape", [(3 * 128 + 1, 2 * 256 + 100), (2 * 128 + 70, 5 * 256), (4 * 128, 24 * 256 + 4)],
                         ids=["last_row_shorter_than_order", "partial_rows", "wide_partial_column"])
def test_neighbour_form_against_the_full_scans_and_the_oracle(coeff, clamped, planes, shape):
    scans = rc.xy_pm(getattr(rc, coeff))
    # offset: the B-spline prefilter is a high-pass; around a level of 4 its result stays away from zero, where the strict
    # relative error between the two forms is meaningful
    imgs = [rc.random_image(shape, np.float32, 70 + p) + np.float32(4.0) for p in range(planes)]
    flags = TILED | capi.RF_PLAN_TILE_ROWS(128)
    nb, names, taken, tiles = _run(shape, scans, clamped, imgs, flags, inplace=(planes == 3))
    full, full_names, full_taken, _ = _run(shape, scans, clamped, imgs, flags | FULL)
    assert tiles[:2] == (256, 128)
    assert taken == (True, True) and full_taken == (False, False)
    assert names == ["fused_tails", "xscan_rows", "fused_pass2"], names
    assert "carry_y" in full_names
    for a, b, im in zip(nb, full, imgs):
        assert _strict(a, b) <= 1e-6
        want = oracle.apply_filter(im.astype(np.float64), scans, clamped)
        assert rc.rel_err(a, want) < 1e-4
        assert rc.rel_err(b, want) < 1e-4


@pytest.mark.parametrize("case", ["running_sum", "pole_097", "gauss2_64_rows", "flag"])
def test_launches_follow_the_decision(case):
    """The launch list of a step has a carry_x / carry_y launch exactly where the plan's decision keeps the scans (wide rows:
    more tiles per row than xscan_rows completes by itself)."""
    shape = (256, 40 * 256)
    scans, flags, want = rc.xy_pm(rc.GAUSS2), TILED | capi.RF_PLAN_TILE_ROWS(128), (True, True)
    if case == "running_sum":
        scans, want = [(0, True, [1.0, 1.0]), (1, True, [1.0, 1.0])], (False, False)
    elif case == "pole_097":
        scans, want = [(0, True, [0.03, 0.97]), (0, False, [0.03, 0.97]), (1, True, [0.03, 0.97])], (False, False)
    elif case == "gauss2_64_rows":
        flags, want = TILED | capi.RF_PLAN_TILE_ROWS(64), (True, False)
    else:
        flags, want = flags | FULL, (False, False)
    imgs = [rc.random_image(shape, np.float32, 80)]
    got, names, taken, _ = _run(shape, scans, case != "running_sum", imgs, flags)
    assert taken == want
    assert ("carry_x" in names) == (not taken[0]), names
    assert ("carry_y" in names) == (not taken[1]), names
    want_img = oracle.apply_filter(imgs[0].astype(np.float64), scans, case != "running_sum")
    assert rc.rel_err(got[0], want_img) < 1e-4


def test_cfg3_16384_three_launches_against_the_oracle_strict():
    """The headline configuration at full size: three launches per step, every pixel against the f64 oracle (strict metric)."""
    c = rc.BASELINE_CONFIGS["cfg3_gaussian2_xy"]
    img = rc.random_image(c["shape"], np.float32, 9)
    got, names, taken, tiles = _run(c["shape"], c["scans"], c["clamped"], [img], 0)
    assert taken == (True, True) and tiles[:2] == (256, 128)
    assert names == ["fused_tails", "xscan_rows", "fused_pass2"], names
    try:
        threads = len(os.sched_getaffinity(0))
    except AttributeError:
        threads = os.cpu_count() or 1
    want = oracle.apply_filter(img.astype(np.float64), c["scans"], c["clamped"], threads=max(1, min(threads, oracle.max_threads(), 64)))
    worst = 0.0
    for r in range(0, img.shape[0], 512):
        worst = max(worst, rc.rel_err_strict(got[0][r:r + 512], want[r:r + 512]))
    assert worst < 1e-4
