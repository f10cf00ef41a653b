"""Volumes of 16-bit float pixels (RF_F16, RF_BF16) on the host.  A volume whose z stage runs on the strided kernels is NATIVE:
the x/y stage's result waits in an f32 volume of the plan's own, so the plan is the f32 plan of the same description with two
first passes (RF_PLAN_STAGED_PASS1) -- launch for launch, tile for tile, table for table -- plus that volume, and nothing is
rounded before the final z pass stores.  Everything else stays staged through f32 planes (convert_in / convert_out: two more
launches), or unsupported where it was."""
import numpy as np
import pytest

import ref_cases as rc
import recfilter_amd as rfa
from recfilter_amd import capi

HOST = dict(device=capi.RF_DEVICE_HOST_ONLY)
FUSED, AUTO = capi.RF_PATH_TILED_FUSED, capi.RF_PATH_AUTO
TILED = capi.RF_PLAN_TILED_ONLY
TWO_PASSES = capi.RF_PLAN_STAGED_PASS1


def _dtypes():
    import torch
    return [("f16", torch.float16), ("bf16", torch.bfloat16)]


DTYPES = _dtypes()
IDS = [d[0] for d in DTYPES]
SHAPE = (64, 96, 128)


def _xyz(coeff=rc.GAUSS2):
    return rc.xy_pm(coeff) + [(2, True, coeff), (2, False, coeff)]


def _f32_count(shape, scans, **kw):
    flags = kw.pop("flags", TILED) | TWO_PASSES
    with rfa.Plan(shape, scans, dtype=np.float32, flags=flags, **kw, **HOST) as p32:
        return p32.num_kernels


@pytest.mark.parametrize("name,tdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("planes", [1, 3])
def test_native_volume_is_the_f32_plan(name, tdt, coeff, clamped, planes):
    scans = _xyz(getattr(rc, coeff))
    with rfa.Plan(SHAPE, scans, dtype=tdt, clamped=clamped, planes=planes, path=FUSED, flags=TILED, **HOST) as p16, \
         rfa.Plan(SHAPE, scans, dtype=np.float32, clamped=clamped, planes=planes, path=FUSED, flags=TILED | TWO_PASSES, **HOST) as p32:
        assert p16.num_kernels == p32.num_kernels          # (the staged form: two more)
        assert p16.path == FUSED and p32.path == FUSED
        assert p16.tiles == p32.tiles
        assert np.array_equal(p16.table("scans"), p32.table("scans"))
        for t in ("H_x", "H_y", "W_x", "A_y", "W_z", "A_z"):
            assert np.array_equal(p16.table(t), p32.table(t))
        # the f32 volume between the two stages, one per Tuple plane, counted by a host-only plan too
        assert p16.workspace_bytes >= 4 * int(np.prod(SHAPE)) * planes
        assert p16.workspace_bytes >= p32.workspace_bytes + 4 * int(np.prod(SHAPE)) * planes


@pytest.mark.parametrize("name,tdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("planes_tile", [32, 64, 128])
def test_native_volume_takes_the_callers_z_tile(name, tdt, planes_tile):
    flags = TILED | capi.RF_PLAN_TILE_PLANES(planes_tile)
    with rfa.Plan((128, 64, 256), _xyz(), dtype=tdt, path=FUSED, flags=flags, **HOST) as p16:
        assert p16.tiles[2] == planes_tile
        assert p16.num_kernels == _f32_count((128, 64, 256), _xyz(), path=FUSED, flags=flags)


@pytest.mark.parametrize("name,tdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("why", ["stage_half", "inplace_z", "walk_pass1", "epilogue", "no_strided_tile", "z_unfiltered"])
def test_staged_again(name, tdt, why):
    shape, scans, kw, flags = SHAPE, _xyz(), {}, TILED
    if why == "stage_half":
        flags |= capi.RF_PLAN_STAGE_HALF
    elif why == "inplace_z":
        flags |= capi.RF_PLAN_INPLACE_Z
    elif why == "walk_pass1":
        flags |= capi.RF_PLAN_WALK_PASS1
    elif why == "epilogue":
        kw["epilogue"] = (0.5, 0.0, 0.25)
    elif why == "no_strided_tile":
        shape = (48, 96, 128)
    elif why == "z_unfiltered":
        scans = rc.xy_pm(rc.GAUSS2)
    with rfa.Plan(shape, scans, dtype=tdt, path=FUSED, flags=flags, **kw, **HOST) as p16, \
         rfa.Plan(shape, scans, dtype=tdt, path=FUSED, flags=flags | capi.RF_PLAN_STAGE_HALF, **kw, **HOST) as forced, \
         rfa.Plan(shape, scans, dtype=np.float32, path=FUSED, flags=flags, **kw, **HOST) as p32:
        # the staged form is what RF_PLAN_STAGE_HALF gives: convert_in + the f32 plan's launches + convert_out
        assert p16.num_kernels == forced.num_kernels and p16.workspace_bytes == forced.workspace_bytes
        # (a z extent without a strided tile runs the generic z stage, whose f32 plan also counts "generic_carry_z_apply": the
        #  exchange structure of the outermost dimension, which adds nothing on one slab and which a staged plan never relayed
        #  -- there the staged count is one above the f32 plan's count, as it was before volumes could be native)
        assert p16.num_kernels == p32.num_kernels + (1 if why == "no_strided_tile" else 2)
        assert p16.workspace_bytes >= p32.workspace_bytes + 4 * int(np.prod(shape))


@pytest.mark.parametrize("name,tdt", DTYPES, ids=IDS)
def test_unchanged_refusals(name, tdt):
    with pytest.raises(capi.RecFilterError) as e:
        rfa.Plan(SHAPE, _xyz(), dtype=tdt, path=FUSED, flags=TILED, shard_rank=0, shard_world=2, **HOST)
    assert e.value.status == capi.RF_ERR_UNSUPPORTED
    with pytest.raises(capi.RecFilterError) as e:
        rfa.Plan(SHAPE, _xyz(), dtype=tdt, path=FUSED, flags=TILED, input_dtype=np.uint8, **HOST)
    assert e.value.status == capi.RF_ERR_UNSUPPORTED


@pytest.mark.parametrize("name,tdt", DTYPES, ids=IDS)
def test_automatic_path(name, tdt):
    """RF_PATH_AUTO: staged below the threshold plan.cpp states (kHalfVolumeNativeSamples), native from it on"""
    scans = _xyz()
    with rfa.Plan(SHAPE, scans, dtype=tdt, path=AUTO, flags=TILED, **HOST) as small, \
         rfa.Plan(SHAPE, scans, dtype=np.float32, path=AUTO, flags=TILED, **HOST) as small32:
        assert small.num_kernels == small32.num_kernels + 2
    big = (512, 512, 1024)
    with rfa.Plan(big, scans, dtype=tdt, path=AUTO, flags=0, **HOST) as p16:
        assert p16.path == FUSED
        assert p16.num_kernels == _f32_count(big, scans, path=AUTO, flags=0)
        assert p16.workspace_bytes >= 4 * int(np.prod(big))
        with rfa.Plan(big, scans, dtype=np.float32, path=AUTO, flags=TWO_PASSES, **HOST) as p32:
            assert p16.tiles == p32.tiles


@pytest.mark.parametrize("name,tdt", DTYPES, ids=IDS)
def test_odd_width_stays_staged(name, tdt):
    shape = (64, 96, 130)
    with rfa.Plan(shape, _xyz(), dtype=tdt, path=AUTO, flags=TILED, **HOST) as p16, \
         rfa.Plan(shape, _xyz(), dtype=np.float32, path=AUTO, flags=TILED, **HOST) as p32:
        assert p16.num_kernels == p32.num_kernels + 2
