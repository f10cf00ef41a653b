"""Native volumes of 16-bit float pixels (RF_F16, RF_BF16) on the GPU: the x/y stage's result waits in an f32 volume of the
plan's own, the final z pass rounds once as it stores.  The two assertions, and their bars, are those of
tests/test_gpu_half_pixels.py (the bars come from the 2-D feature, not from this code):

  1. against the f64 oracle of the widened input:  rel_err < 1e-4 + eps, eps = 2^-11 (f16) / 2^-8 (bf16);
  2. against torch's rounding of the F32 plan's result for the widened input (same flags + RF_PLAN_STAGED_PASS1, i.e. the plan
     the native one mirrors): bit patterns differ by at most 1, at least 98 % identical, on positive results.

Every case also asserts the launch list: no convert_* step, and name for name the f32 plan's."""
import numpy as np
import pytest

import oracle
import ref_cases as rc
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

TILED = capi.RF_PLAN_TILED_ONLY
FUSED = capi.RF_PATH_TILED_FUSED
AUTO = capi.RF_PATH_AUTO
TWO_PASSES = capi.RF_PLAN_STAGED_PASS1
KINDS = ["f16", "bf16"]
Z_PAIR, Z_CAUSAL, Z_ANTICAUSAL = "z_pair", "z_causal", "z_anticausal"        # PAT 2 / 1 / 0 of the strided kernels


def _types():
    import torch
    return {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8)}


def _narrow(img, kind):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(_types()[kind][0])


def _scans(coeff, z):
    zs = {Z_PAIR: [(2, True, coeff), (2, False, coeff)], Z_CAUSAL: [(2, True, coeff)], Z_ANTICAUSAL: [(2, False, coeff)]}[z]
    return rc.xy_pm(coeff) + zs


def _run(shape, scans, clamped, ins, dtype, path=FUSED, flags=TILED, inplace=False, **kw):
    """ins: CPU torch tensors of the plan's type.  Returns (outputs on the CPU, launch names, path, tiles, workspace bytes)."""
    import recfilter_amd as rfa
    with rfa.Plan(shape, scans, dtype=dtype, clamped=clamped, planes=len(ins), path=path, flags=flags, **kw) as plan:
        dev = [t.cuda() for t in ins]
        if inplace:
            _, timed = plan.execute_timed(dev, dev)
            outs = dev
        else:
            outs, timed = plan.execute_timed(dev)
        got = [o.cpu() for o in outs]
        return got, [n for n, _ in timed], plan.path, plan.tiles, plan.workspace_bytes


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).to(torch.int32)


def _assert_one_rounding(got16, ref32, kind, what=""):
    """assertion 2: got16 against torch's rounding of the f32 plan's result"""
    ref16 = ref32.to(_types()[kind][0])
    assert bool((ref32 > 0).all()), "the case is built to give positive results"
    d = (_bits(got16) - _bits(ref16)).abs()
    worst, same = int(d.max()), float((d == 0).double().mean())
    print(f"{what} {kind}: max bit difference {worst}, identical {100.0 * same:.4f} %")
    assert worst <= 1
    assert same >= 0.98


def _assert_oracle(got16, in16, scans, clamped, kind, want=None):
    """assertion 1: got16 against the f64 oracle of the widened input"""
    if want is None:
        want = oracle.apply_filter(in16.float().numpy().astype(np.float64), scans, clamped)
    err = rc.rel_err(got16.float().numpy(), want)
    bar = 1e-4 + _types()[kind][1]
    print(f"{kind}: rel err {err:.4e} against {bar:.4e}")
    assert err < bar


def _both(shape, scans, clamped, imgs, kind, path=FUSED, flags=TILED, inplace=False, want=None, **kw):
    """the 16-bit plan and the f32 plan (two first passes) of the widened input: both assertions and the launch list"""
    import torch
    tdt = _types()[kind][0]
    in16 = [_narrow(im, kind) for im in imgs]
    got, names, path16, tiles, ws = _run(shape, scans, clamped, in16, tdt, path, flags, inplace, **kw)
    ref, names32, _, tiles32, _ = _run(shape, scans, clamped, [t.float() for t in in16], torch.float32, path, flags | TWO_PASSES, inplace, **kw)
    print(f"{kind} {shape}: tiles {tiles} launches {names}")
    assert path16 == FUSED
    assert not any(n.startswith("convert") for n in names), names
    assert names == names32, (names, names32)
    assert tiles == tiles32
    assert ws >= 4 * int(np.prod(shape)) * len(imgs)
    for i, (g, r, x) in enumerate(zip(got, ref, in16)):
        assert g.dtype == tdt
        _assert_one_rounding(g, r, kind)
        _assert_oracle(g, x, scans, clamped, kind, want=want[i] if want is not None else None)
    return dict(names=names, tiles=tiles)


# shape (z, y, x) -> which instances it takes: (64, 128, 512) whole x/y tiles and the UNI strided instances (x * y a multiple
# of 256 lines in runs of 256); (64, 96, 128) a partial tile column, UNI; (96, 200, 260) partial tiles both ways and the
# general strided instance
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("shape", [(64, 128, 512), (64, 96, 128), (96, 200, 260)], ids=["whole_uni", "partial_uni", "partial_general"])
def test_native_volume(kind, coeff, clamped, shape):
    scans = _scans(getattr(rc, coeff), Z_PAIR)
    info = _both(shape, scans, clamped, [rc.random_image(shape, np.float32, 90)], kind)
    assert info["tiles"][0] == 256


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("z", [Z_CAUSAL, Z_ANTICAUSAL])
@pytest.mark.parametrize("shape", [(64, 128, 512), (96, 200, 260)], ids=["uni", "general"])
def test_other_z_scan_patterns(kind, z, shape):
    scans = _scans(rc.GAUSS2, z)
    _both(shape, scans, True, [rc.random_image(shape, np.float32, 91)], kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tz", [32, 64, 128])
@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3"])
def test_z_tile_widths(kind, tz, coeff):
    shape = (256, 64, 256)
    info = _both(shape, _scans(getattr(rc, coeff), Z_PAIR), True, [rc.random_image(shape, np.float32, 92)], kind,
                 flags=TILED | capi.RF_PLAN_TILE_PLANES(tz))
    assert info["tiles"][2] == tz


ORDER1 = [0.5, 0.5]        # y = (x + y_prev) / 2: positive impulse response, unit gain


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("coeff", ["ORDER1", "GAUSS2", "GAUSS3"])
@pytest.mark.parametrize("rows,shape", [(128, (32, 2 * 128 + 40, 2 * 256 + 8)), (128, (32, 256, 512)), (64, (32, 3 * 64, 256)),
                                        (64, (32, 64 + 20, 256 + 8)), (32, (64, 96, 256)), (32, (32, 40, 260))],
                         ids=["rows128_partial", "rows128_whole", "rows64", "rows64_partial", "rows32", "rows32_partial"])
def test_xy_tile_heights(kind, coeff, rows, shape):
    """the final x/y pass with a 16-bit source and an f32 destination: every order on every tile height, whole tiles (the
    compile-time pair of scans) and partial ones (the EDGE instances, the strips of the 128-row pass)"""
    w = ORDER1 if coeff == "ORDER1" else getattr(rc, coeff)
    info = _both(shape, _scans(w, Z_PAIR), True, [rc.random_image(shape, np.float32, 93)], kind,
                 flags=TILED | capi.RF_PLAN_TILE_ROWS(rows))
    assert info["tiles"][1] == rows


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,shape", [(128, (32, 256, 256)), (64, (32, 128, 256)), (32, (32, 64, 256))], ids=["rows128", "rows64", "rows32"])
@pytest.mark.parametrize("coeff", ["ORDER1", "GAUSS3"])
def test_general_xy_pattern_on_whole_tiles(kind, rows, shape, coeff):
    """x/y scans that are not the usual pair, on whole tiles: the general-pattern instances of every tile height"""
    w = ORDER1 if coeff == "ORDER1" else getattr(rc, coeff)
    scans = [(0, True, w), (1, True, w), (2, True, w), (2, False, w)]
    info = _both(shape, scans, True, [rc.random_image(shape, np.float32, 89)], kind, flags=TILED | capi.RF_PLAN_TILE_ROWS(rows))
    assert info["tiles"][1] == rows


@pytest.mark.parametrize("kind", KINDS)
def test_order_one_and_a_general_xy_pattern(kind):
    """order 1, and x/y scans that are not the usual pair (the general-pattern final x/y pass)"""
    shape = (64, 128, 256)
    smooth = [1.0 - 0.5, 0.5]         # (positive impulse response, unit gain)
    scans = [(0, True, smooth), (1, False, smooth), (1, True, smooth), (2, True, smooth), (2, False, smooth)]
    _both(shape, scans, True, [rc.random_image(shape, np.float32, 94)], kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_three_planes(kind, inplace):
    shape = (64, 96, 128)
    imgs = [rc.random_image(shape, np.float32, 95 + p) for p in range(3)]
    _both(shape, _scans(rc.GAUSS2, Z_PAIR), True, imgs, kind, inplace=inplace)


@pytest.mark.parametrize("kind", KINDS)
def test_in_place_one_plane(kind):
    shape = (64, 128, 512)
    _both(shape, _scans(rc.GAUSS3, Z_PAIR), False, [rc.random_image(shape, np.float32, 98)], kind, inplace=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(64, 128, 512), (96, 200, 260)], ids=["whole", "partial"])
def test_prologue(kind, shape):
    """x' = x / 255 + 1/16 applied as the samples arrive, in both x/y passes (integers up to 255 are exact in both types)"""
    scans = _scans(rc.GAUSS2, Z_PAIR)
    img = np.floor(rc.random_image(shape, np.float32, 99) * 255.0).astype(np.float32)
    pre = (1.0 / 255.0, 0.0625)
    x = _narrow(img, kind).float().numpy().astype(np.float64)
    want = oracle.apply_filter(x * np.float64(np.float32(pre[0])) + pre[1], scans, True)
    _both(shape, scans, True, [img], kind, want=[want], prologue=pre)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(64, 256, 512), (32, 200, 516)], ids=["whole_tiles", "partial_tiles"])
def test_summed_volume_table_is_exact(kind, shape):
    """Integers 0..3 are exact in both types and every partial sum stays below 2^24, so the f32 result is exact in any summation
    order: the output is torch's rounding of the exact table, bit for bit -- +inf above 65504 in binary16 included.  The 2-D
    partial sums pass 2048, where consecutive integers stop being binary16 (256: bfloat16) values: an x/y result rounded to 16
    bits anywhere on its way to the z stage fails this."""
    import torch
    tdt = _types()[kind][0]
    img = np.random.default_rng(100).integers(0, 4, size=shape).astype(np.float32)
    scans = [(0, True, [1.0, 1.0]), (1, True, [1.0, 1.0]), (2, True, [1.0, 1.0])]
    got, names, path, _, _ = _run(shape, scans, False, [_narrow(img, kind)], tdt)
    plane = np.cumsum(np.cumsum(img.astype(np.float64), axis=1), axis=2)
    exact = np.cumsum(plane, axis=0)
    assert plane.max() > 2048 and exact.max() < 2 ** 24
    want = torch.from_numpy(exact.astype(np.float32)).to(tdt)
    assert path == FUSED and not any(n.startswith("convert") for n in names), names
    assert torch.equal(_bits(got[0]), _bits(want))
    if kind == "f16":
        assert bool(torch.isinf(got[0]).any())


@pytest.mark.parametrize("kind", KINDS)
def test_full_size_on_the_automatic_path(kind, shipped_defaults):
    """2^28 samples under RF_PATH_AUTO with flags = 0: native, assertion 2 against the f32 plan with two first passes (the f64
    oracle of such a volume would take minutes on the CPU)"""
    import torch
    import recfilter_amd as rfa
    shape = (512, 512, 1024)
    tdt = _types()[kind][0]
    scans = _scans(rc.GAUSS2, Z_PAIR)
    x16 = rc.cuda_image(shape, np.float32, 101).to(tdt)
    with rfa.Plan(shape, scans, dtype=tdt, clamped=True, path=AUTO, flags=0) as p16:
        got, timed = p16.execute_timed([x16])
        names = [n for n, _ in timed]
        assert p16.path == FUSED
    with rfa.Plan(shape, scans, dtype=torch.float32, clamped=True, path=AUTO, flags=TWO_PASSES) as p32:
        ref, timed32 = p32.execute_timed([x16.float()])
    assert not any(n.startswith("convert") for n in names), names
    assert names == [n for n, _ in timed32], names
    assert bool((ref[0] > 0).all())
    ref16 = ref[0].to(tdt)
    del ref
    d = (got[0].view(torch.int16).to(torch.int32) - ref16.view(torch.int16).to(torch.int32)).abs()
    worst, same = int(d.max()), float((d == 0).double().mean())
    print(f"2^28 {kind}: max bit difference {worst}, identical {100.0 * same:.4f} %")
    assert worst <= 1 and same >= 0.98
