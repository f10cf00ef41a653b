"""The row-scan form of the neighbour-form step (plan_fused.cpp, row_scans), checked without a GPU.

Where both dimensions of an order-2 f32 plan of whole 256 x 128 tiles take the neighbour form, pass 1 runs the tile-local x scans
of the combined rows itself, the launch between the passes (still the step "xscan_rows") only contracts the x tails into tau,
and the final pass completes every carry it loads.  Here:
  * the decision rf_plan_table("row_scans") reports on host-only plans, and that it moves neither the workspace nor the
    number of launches;
  * the rearranged algebra: tests/row_scans_emulator.py against the neighbour-form emulator and against the f64 oracle."""
import numpy as np
import pytest

import oracle
import ref_cases as rc
import recfilter_amd as rfa
from recfilter_amd import capi
from row_scans_emulator import RowScansEmu
from test_neighbour_carries_host import NeighbourEmu

HOST = dict(device=capi.RF_DEVICE_HOST_ONLY)
FUSED = capi.RF_PATH_TILED_FUSED
SEPARATE = capi.RF_PLAN_SEPARATE_ROW_SCANS
ROWS128 = capi.RF_PLAN_TILE_ROWS(128)
G2 = rc.xy_pm(rc.GAUSS2)


def _taken(plan):
    t = plan.table("row_scans")
    assert t.shape == (1,)
    return bool(t[0])


def test_cfg3_takes_the_row_scan_form():
    c = rc.BASELINE_CONFIGS["cfg3_gaussian2_xy"]
    assert c["shape"] == (16384, 16384)
    with rfa.Plan(c["shape"], c["scans"], clamped=c["clamped"], path=FUSED, **HOST) as plan, \
         rfa.Plan(c["shape"], c["scans"], clamped=c["clamped"], path=FUSED, flags=SEPARATE, **HOST) as kept:
        assert plan.tiles[:2] == (256, 128)
        assert _taken(plan) and not _taken(kept)
        # the form changes which kernels the three steps launch, nothing else
        assert plan.workspace_bytes == kept.workspace_bytes
        assert plan.num_kernels == kept.num_kernels == 3
        assert list(plan.table("neighbour_carries")) == list(kept.table("neighbour_carries"))


@pytest.mark.parametrize("case", ["flag", "gauss3", "bicubic", "partial_tiles", "rows64", "f16", "byte_output", "sharded", "volume"])
def test_everything_else_keeps_the_three_kernels(case):
    shape, scans, kw = (1024, 2048), G2, dict(clamped=True, path=FUSED, flags=ROWS128)
    if case == "flag":
        kw["flags"] = ROWS128 | SEPARATE
    elif case == "gauss3":
        scans = rc.xy_pm(rc.GAUSS3)
    elif case == "bicubic":
        scans = rc.xy_pm(rc.BICUBIC_COEFF)
    elif case == "partial_tiles":
        shape = (385, 612)
    elif case == "rows64":
        kw["flags"] = capi.RF_PLAN_TILE_ROWS(64)
    elif case == "f16":
        kw["dtype"] = np.float16
    elif case == "byte_output":
        kw.update(dtype=np.float32, input_dtype=np.uint8, output_dtype=np.uint8)
    elif case == "sharded":
        kw.update(shard_rank=0, shard_world=2, flags=0)
    elif case == "volume":
        shape, scans, kw["flags"] = (64, 1024, 1024), G2 + [(2, True, rc.GAUSS2)], 0
    with rfa.Plan(shape, scans, **kw, **HOST) as plan:
        assert plan.path_name == "tiled_fused"
        assert not _taken(plan)
    if case in ("flag", "gauss3", "bicubic", "partial_tiles"):
        # ... and with the flag the same plan still takes the neighbour form (the flag is not RF_PLAN_FULL_CARRY_SCAN)
        with rfa.Plan(shape, scans, **kw, **HOST) as plan:
            assert plan.tiles[1] == 128
            _, tx, _, ty = plan.table("neighbour_carries")
            assert tx and ty


@pytest.mark.parametrize("shape", [(128, 256), (128, 512), (256, 256), (384, 768), (1024, 2048)])
def test_flag_moves_neither_workspace_nor_launches(shape):
    with rfa.Plan(shape, G2, clamped=True, path=FUSED, flags=ROWS128, **HOST) as plan, \
         rfa.Plan(shape, G2, clamped=True, path=FUSED, flags=ROWS128 | SEPARATE, **HOST) as kept:
        assert _taken(plan) and not _taken(kept)
        assert plan.workspace_bytes == kept.workspace_bytes
        assert plan.num_kernels == kept.num_kernels
    with rfa.Plan(shape, G2, clamped=True, planes=3, path=FUSED, flags=ROWS128, **HOST) as plan, \
         rfa.Plan(shape, G2, clamped=True, planes=3, path=FUSED, flags=ROWS128 | SEPARATE, **HOST) as kept:
        assert _taken(plan) and not _taken(kept)
        assert plan.workspace_bytes == kept.workspace_bytes
        assert plan.num_kernels == kept.num_kernels


@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("shape", [(128, 256), (128, 512), (256, 256), (384, 768)])
def test_row_scan_emulator_matches_the_neighbour_form_and_the_oracle(shape, clamped):
    img = rc.random_image(shape, np.float32, 61)
    with rfa.Plan(shape, G2, clamped=clamped, path=FUSED, flags=ROWS128, **HOST) as plan:
        assert plan.tiles[:2] == (256, 128) and _taken(plan)
        nb = NeighbourEmu(plan, G2, clamped).run(img)
        rs = RowScansEmu(plan, G2, clamped).run(img)
        rs32 = RowScansEmu(plan, G2, clamped, round_f32=True).run(img)
    want = oracle.apply_filter(img.astype(np.float64), G2, clamped)
    peak = float(np.max(np.abs(nb)))
    diff = float(np.max(np.abs(rs - nb)))
    print(f"{shape} clamped={clamped}: row scans against neighbour form {diff / peak:.3e} of the peak; "
          f"rel err f64 {rc.rel_err(rs, want):.3e}, stored values in f32 {rc.rel_err(rs32, want):.3e}")
    assert diff <= 1e-9 * peak              # f64 emulators of the same sums in another order
    assert rc.rel_err(rs, want) < 1e-4
    assert rc.rel_err(rs32, want) < 1e-4    # every stored tail, row and tau rounded to f32
