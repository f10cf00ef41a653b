"""Byte volumes (RF_IO_U8, three dimensions) on the host: which volumes are native, that a native plan is the RF_IN_U8 plan of
the same description with two first passes (RF_PLAN_STAGED_PASS1) plus one f32 volume per plane and minus its stand-alone
epilogue, which volumes stay staged or refused, and that the per-sample rule of tests/test_gpu_u8_volumes.py is one a correct
f32 implementation passes on the very inputs of that test.

A host-only plan cannot be executed and the library names its launches only as it runs them (rf_plan_execute_timed), so the
host side sees the launch list as a COUNT: "the RF_IN_U8 plan's launches minus pointwise_post, no convert_* step" is asserted
here as num_kernels, and name for name by tests/test_gpu_u8_volumes.py (_assert_native) for the same shapes."""
import numpy as np
import pytest

import recfilter_amd as rfa
import ref_cases as rc
import u8_cases as u8
import u8_volume_cases as vc
from recfilter_amd import capi

HOST = dict(device=capi.RF_DEVICE_HOST_ONLY)
TILED, FUSED, AUTO, IO, IN = vc.TILED, vc.FUSED, vc.AUTO, vc.IO, vc.IN
TWO_PASSES = capi.RF_PLAN_STAGED_PASS1
XYZ = vc.scans_of(rc.GAUSS2, "pair")


def _pair(shape, scans, flags=TILED, path=FUSED, in_flags=None, **kw):
    """(byte plan, RF_IN_U8 plan) of one description, host-only"""
    p8 = rfa.Plan(shape, scans, path=path, flags=flags, **IO, **kw, **HOST)
    pin = rfa.Plan(shape, scans, path=path, flags=flags if in_flags is None else in_flags, **IN, **kw, **HOST)
    return p8, pin


@pytest.mark.parametrize("shape", vc.SHAPES, ids=str)
@pytest.mark.parametrize("zpat", vc.Z_PATTERNS)
@pytest.mark.parametrize("setup", vc.SETUPS, ids=vc.SETUP_IDS)
@pytest.mark.parametrize("planes", [1, 3])
def test_native_volume_is_the_u8_input_plan(shape, zpat, setup, planes):
    _, prologue, epilogue = setup
    p8, pin = _pair(shape, vc.scans_of(rc.GAUSS2, zpat), in_flags=TILED | TWO_PASSES, clamped=True, planes=planes,
                    prologue=prologue, epilogue=epilogue)
    with p8, pin:
        assert p8.path == FUSED and pin.path == FUSED
        # launch for launch (no convert_out), without the stand-alone pointwise_post: the affine epilogue rides on the final store
        assert p8.num_kernels == pin.num_kernels - (1 if epilogue is not None else 0)
        assert p8.tiles == pin.tiles
        for t in ("H_x", "H_y", "W_x", "A_y", "W_z", "A_z", "scans"):
            assert np.array_equal(p8.table(t), pin.table(t)), t
        # the f32 volume between the two stages, one per plane, counted by a host-only plan and listed as scratch
        samples = int(np.prod(shape))
        assert p8.workspace_bytes >= pin.workspace_bytes + 4 * samples * planes
        assert sum(1 for _, kind, n in p8.debug_buffers() if kind == "scratch" and n == 4 * samples) >= planes


@pytest.mark.parametrize("coeff", ["GAUSS3", "ORDER1"])
def test_native_volume_orders(coeff):
    c = vc.ORDER1 if coeff == "ORDER1" else rc.GAUSS3
    p8, pin = _pair((64, 96, 128), vc.scans_of(c, "pair"), in_flags=TILED | TWO_PASSES)
    with p8, pin:
        assert p8.num_kernels == pin.num_kernels and p8.workspace_bytes >= pin.workspace_bytes + 4 * 64 * 96 * 128


@pytest.mark.parametrize("planes_tile", [32, 64, 128])
def test_native_volume_takes_the_callers_z_tile(planes_tile):
    flags = TILED | capi.RF_PLAN_TILE_PLANES(planes_tile)
    p8, pin = _pair((256, 64, 256), XYZ, flags=flags, in_flags=flags | TWO_PASSES)
    with p8, pin:
        assert p8.tiles[2] == planes_tile and p8.tiles == pin.tiles and p8.num_kernels == pin.num_kernels


@pytest.mark.parametrize("why", ["depth_40", "odd_width", "input_operand", "stage_half", "inplace_z", "walk_pass1", "auto_small",
                                 "z_unfiltered", "z_alone", "order_4"])
def test_excluded_volumes_stay_staged(why):
    """one launch (convert_out) and one f32 plane per image plane more than the RF_IN_U8 plan of the same description"""
    shape, scans, flags, path, kw = (64, 96, 128), XYZ, TILED, FUSED, {}
    if why == "depth_40":
        shape = (40, 96, 128)
    elif why == "odd_width":
        shape, path = (64, 96, 130), AUTO            # (the fused path refuses the RF_IN_U8 plan of such a width as well)
    elif why == "input_operand":
        kw["epilogue"] = (-1.0, 2.0, 0.0)
    elif why == "stage_half":
        flags |= capi.RF_PLAN_STAGE_HALF
    elif why == "inplace_z":
        flags |= capi.RF_PLAN_INPLACE_Z
    elif why == "walk_pass1":
        flags |= capi.RF_PLAN_WALK_PASS1
    elif why == "auto_small":
        path = AUTO                                  # 2^19.6 samples: below the threshold of RF_PATH_AUTO
    elif why == "z_unfiltered":
        scans = rc.xy_pm(rc.GAUSS2)
    elif why == "z_alone":
        scans, path = [(2, True, rc.GAUSS2), (2, False, rc.GAUSS2)], AUTO
    elif why == "order_4":
        scans, path = XYZ + [(2, True, [0.1, 0.4, 0.3, 0.1, 0.1])], AUTO
    in_flags = flags & ~capi.RF_PLAN_STAGE_HALF
    p8, pin = _pair(shape, scans, flags=flags, path=path, in_flags=in_flags, **kw)
    with p8, pin:
        samples = int(np.prod(shape))
        assert p8.workspace_bytes == pin.workspace_bytes + 4 * samples
        assert p8.path == pin.path
        if why != "depth_40":
            assert p8.num_kernels == pin.num_kernels + 1
        else:
            # (a depth without a strided tile runs the generic z stage, whose plan also counts the apply step of the outermost
            #  dimension's exchange structure; the staged plan lists what one device runs -- tests/test_half_volumes_host.py)
            assert p8.num_kernels in (pin.num_kernels, pin.num_kernels + 1)


def test_automatic_path_takes_the_native_form_from_the_threshold_on():
    big = (256, 256, 256)            # 2^24 samples per plane
    p8, pin = _pair(big, XYZ, flags=0, path=AUTO, in_flags=TWO_PASSES)
    with p8, pin:
        assert p8.path == FUSED and p8.num_kernels == pin.num_kernels and p8.tiles == pin.tiles
        assert p8.workspace_bytes >= pin.workspace_bytes + 4 * int(np.prod(big))
    with rfa.Plan(big, XYZ, path=AUTO, flags=capi.RF_PLAN_STAGE_HALF, **IO, **HOST) as staged, \
         rfa.Plan(big, XYZ, path=AUTO, flags=0, **IN, **HOST) as pin:
        assert staged.num_kernels == pin.num_kernels + 1


def test_two_dimensional_rule_is_unchanged():
    scans = rc.xy_pm(rc.GAUSS2)
    with rfa.Plan((512, 1024), scans, clamped=True, flags=TILED, **IO, **HOST) as p8, \
         rfa.Plan((512, 1024), scans, clamped=True, flags=TILED, **IN, **HOST) as pin:
        assert p8.num_kernels == pin.num_kernels and p8.workspace_bytes == pin.workspace_bytes


def test_sharded_volumes_are_refused():
    for kw in (dict(shard_rank=0, shard_world=2), dict(flags=TILED | capi.RF_PLAN_FORCE_EXCHANGE)):
        with pytest.raises(capi.RecFilterError) as e:
            rfa.Plan((64, 96, 128), XYZ, path=FUSED, **{"flags": TILED, **kw}, **IO, **HOST)
        assert e.value.status == capi.RF_ERR_UNSUPPORTED


def test_plans_without_byte_output_are_unchanged_by_the_volume_rule():
    """RF_PLAN_STAGE_HALF means nothing to a volume that does not store bytes"""
    for extra in (IN, dict(dtype=np.float32)):
        with rfa.Plan((64, 96, 128), XYZ, path=FUSED, flags=TILED | capi.RF_PLAN_STAGE_HALF, **extra, **HOST) as a, \
             rfa.Plan((64, 96, 128), XYZ, path=FUSED, flags=TILED, **extra, **HOST) as b:
            assert a.num_kernels == b.num_kernels and a.workspace_bytes == b.workspace_bytes and a.tiles == b.tiles


# ---- the rule of the GPU test is one a correct f32 implementation passes --------------------------------------------------
@pytest.mark.parametrize("shape", vc.SHAPES, ids=str)
@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3"])
@pytest.mark.parametrize("zpat", vc.Z_PATTERNS)
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
def test_the_f32_oracle_passes_the_one_rounding_rule(shape, coeff, zpat, clamped):
    """sat8 of the oracle run in f32 obeys |got - clip(want)| <= 0.5 + 1e-4 * scale for every setup, on byte_image(shape,
    seed_of(shape))"""
    scans = vc.scans_of(getattr(rc, coeff), zpat)
    img = u8.byte_image(shape, u8.seed_of(shape))
    for name, prologue, epilogue in vc.SETUPS:
        want, scale = u8.want_and_scale(img, scans, clamped, prologue, epilogue)
        got = u8.f32_reference_bytes(img, scans, clamped, prologue, epilogue)
        excess = u8.rule_excess(got, want, scale)
        assert excess <= 0.0, f"{name}: the f32 oracle misses the rule by {excess}"
