"""The row-scan form of the neighbour-form step on the GPU (plan_fused.cpp, row_scans): mfma_tails_kernel RS scans the combined
rows in pass 1, xtau_kernel (the step "xscan_rows") stores tau, fused_pass2_tall_kernel RS completes its x carries from the raw
tails and adds the residual to the y tails it loads.  RF_PLAN_SEPARATE_ROW_SCANS keeps the three kernels of the neighbour form:
both forms run the same sums in the same order, and both must pass the f64 oracle."""
import functools

import numpy as np
import pytest

import guarded
import oracle
import ref_cases as rc
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

FUSED = capi.RF_PATH_TILED_FUSED
FLAGS = capi.RF_PLAN_TILED_ONLY | capi.RF_PLAN_TILE_ROWS(128)
SEPARATE = capi.RF_PLAN_SEPARATE_ROW_SCANS
G2 = rc.xy_pm(rc.GAUSS2)
NAMES = ["fused_tails", "xscan_rows", "fused_pass2"]

# 384 x 768: one interior tile with all eight neighbours and every border variant; 128 x 256: a single tile (no neighbour, no tau);
# 128 x 512, 256 x 256: border variants only, one dimension each; 256 x 1280: five tiles per row
SHAPES = [(384, 768), (128, 256), (128, 512), (256, 256), (256, 1280)]


@functools.lru_cache(maxsize=None)
def _image(shape, seed):
    # offset as in tests/test_gpu_neighbour_carries.py: away from zero the strict relative difference of two forms is meaningful
    img = rc.random_image(shape, np.float32, seed) + np.float32(4.0)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(shape, seed, clamped):
    want = oracle.apply_filter(_image(shape, seed).astype(np.float64), G2, clamped)
    want.setflags(write=False)
    return want


def _strict(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6)))


def _run(shape, clamped, imgs, flags, inplace):
    import torch
    import recfilter_amd as rfa
    with rfa.Plan(shape, G2, clamped=clamped, planes=len(imgs), path=FUSED, flags=flags) as plan:
        dev = [torch.from_numpy(np.array(im)).cuda() for im in imgs]
        if inplace:
            _, timed = plan.execute_timed(dev, dev)
            outs = dev
        else:
            outs, timed = plan.execute_timed(dev)
        got = [o.cpu().numpy() for o in outs]
        taken = bool(plan.table("row_scans")[0])
        nb = plan.table("neighbour_carries")
        assert plan.tiles[:2] == (256, 128) and nb[1] and nb[3]
    return got, [n for n, _ in timed], taken


@pytest.mark.parametrize("planes", [1, 3], ids=["1_plane", "3_planes_in_place"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_scan_form_against_the_three_kernels_and_the_oracle(shape, clamped, planes):
    seeds = [70 + p for p in range(planes)]
    imgs = [_image(shape, s) for s in seeds]
    rs, rs_names, rs_taken = _run(shape, clamped, imgs, FLAGS, inplace=(planes == 3))
    sep, sep_names, sep_taken = _run(shape, clamped, imgs, FLAGS | SEPARATE, inplace=(planes == 3))
    assert rs_taken and not sep_taken
    assert rs_names == NAMES and sep_names == NAMES, (rs_names, sep_names)
    for a, b, s in zip(rs, sep, seeds):
        d = _strict(a, b)
        print(f"{shape} clamped={clamped} plane seed {s}: row scans against three kernels, strict {d:.3e}"
              f" ({'bit-identical' if np.array_equal(a.view(np.uint32), b.view(np.uint32)) else 'NOT bit-identical'})")
        assert d <= 1e-6
        want = _want(shape, s, clamped)
        assert rc.rel_err(a, want) < 1e-4
        assert rc.rel_err(b, want) < 1e-4


@pytest.mark.parametrize("planes,inplace", [(1, False), (3, True)], ids=["1_plane", "3_planes_in_place"])
def test_guarded_planes_and_poisoned_scratch(planes, inplace):
    """Guarded planes, and a fresh plan whose scratch is all 0xFF before its first execute: bit for bit the plain run's result --
    the row-scan form reads nothing it has not written in the same step, the unused remainder of the allocation that holds tau
    (the completed x tails of the three-kernel form) included."""
    import torch
    import recfilter_amd as rfa
    shape, clamped = (384, 768), True
    A = [torch.from_numpy(np.array(_image(shape, 70 + p))) for p in range(planes)]
    with rfa.Plan(shape, G2, clamped=clamped, planes=planes, path=FUSED, flags=FLAGS) as plan:
        assert bool(plan.table("row_scans")[0])
        plain = [t.cuda() for t in A]
        outs = plain if inplace else None
        res = plan.execute(plain, outs)
        torch.cuda.synchronize()
        r1 = [o.cpu() for o in (plain if inplace else res)]
        got = guarded.guarded_execute(lambda ins, outs: plan.execute(ins, outs), shape, np.float32, np.float32, A, inplace=inplace)
        guarded.assert_bits_equal(got, r1, "guarded planes against plain planes")
    for g, p in zip(got, range(planes)):
        guarded.assert_oracle(g, _want(shape, 70 + p, clamped), "f32")
    with rfa.Plan(shape, G2, clamped=clamped, planes=planes, path=FUSED, flags=FLAGS) as fresh:
        filled = guarded.poisoned_scratch(fresh, A, r1, inplace=inplace)
        assert filled >= 3          # x tails, the tau allocation, y tails
