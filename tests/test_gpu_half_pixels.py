"""16-bit float pixels (RF_F16, RF_BF16) on the GPU.  They are storage types: out = round16(F_f32(widen(in))), one rounding,
to nearest even, at the final store.  Two assertions carry that contract for got16 = the 16-bit plan's output:

  1. against the f64 oracle of the widened input:  rel_err < 1e-4 + eps, eps = 2^-11 (f16) / 2^-8 (bf16) -- the suite's f32
     bar plus half an ulp of the final rounding (derived, not measured);
  2. against ref16 = torch's rounding of the F32 plan's output for the widened input (same flags, same path): the bit patterns
     differ by at most 1 everywhere and at least 98 % of the samples are bit-identical.  A path that rounds an intermediate
     between its x and y stages leaves ~9 % of the samples different, one that truncates 50 % -- and both pass 1.

Native plans (2-D images, long 1-D signals on the fused kernels) list the f32 plan's launches; staged plans (everything
else) show convert_in / convert_out around the f32 plan's launches and own the f32 planes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import ref_cases as rc
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

TILED = capi.RF_PLAN_TILED_ONLY
FUSED = capi.RF_PATH_TILED_FUSED
AUTO = capi.RF_PATH_AUTO
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _types():
    import torch
    return {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8)}


KINDS = ["f16", "bf16"]


def _narrow(img, kind):
    """a host f32 image rounded to the 16-bit type (a CPU torch tensor)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(_types()[kind][0])


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
    import torch
    ref16 = ref32.to(_types()[kind][0])
    assert bool((ref32 > 0).all()), "the case is built to give positive results"
    d = (_bits(got16) - _bits(ref16)).abs()
    worst, same = int(d.max()), float((d == 0).double().mean())
    print(f"{what} {kind}: max bit difference {worst}, identical {100.0 * same:.4f} %")
    assert worst <= 1
    assert same >= 0.98


def _assert_oracle(got16, in16, scans, clamped, kind, want=None, scale=None):
    """assertion 1: got16 against the f64 oracle of the widened input"""
    if want is None:
        want = oracle.apply_filter(in16.float().numpy().astype(np.float64), scans, clamped)
    err = rc.rel_err(got16.float().numpy(), want, scale=scale)
    bar = 1e-4 + _types()[kind][1]
    print(f"{kind}: rel err {err:.4e} against {bar:.4e}")
    assert err < bar


def _both(shape, scans, clamped, imgs, kind, path=FUSED, flags=TILED, inplace=False, oracle_check=True, **kw):
    """runs the 16-bit plan and the f32 plan of the widened input; both assertions; returns what the two plans showed"""
    import torch
    tdt = _types()[kind][0]
    in16 = [_narrow(im, kind) for im in imgs]
    got, names, path16, tiles, ws = _run(shape, scans, clamped, in16, tdt, path, flags, inplace, **kw)
    ref, names32, path32, tiles32, ws32 = _run(shape, scans, clamped, [t.float() for t in in16], torch.float32, path, flags, inplace, **kw)
    for g, r, x in zip(got, ref, in16):
        assert g.dtype == tdt
        _assert_one_rounding(g, r, kind)
        if oracle_check:
            _assert_oracle(g, x, scans, clamped, kind)
    return dict(names=names, names32=names32, path=path16, path32=path32, tiles=tiles, tiles32=tiles32, ws=ws, ws32=ws32)


# ---- native 2-D ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3", "BICUBIC_COEFF"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("shape", [(3 * 128, 4 * 256), (2 * 128 + 70, 5 * 256), (4 * 128, 24 * 256 + 4)],
                         ids=["whole_tiles", "partial_rows", "wide_partial_column"])
def test_native_2d_128_row_tiles(kind, coeff, clamped, planes, shape):
    scans = rc.xy_pm(getattr(rc, coeff))
    # (offset: the B-spline prefilter is a high-pass; around a level of 4 its result stays positive and in binary16's normal range)
    imgs = [rc.random_image(shape, np.float32, 70 + p) + np.float32(4.0 if coeff == "BICUBIC_COEFF" else 0.0) for p in range(planes)]
    info = _both(shape, scans, clamped, imgs, kind, flags=TILED | capi.RF_PLAN_TILE_ROWS(128), inplace=(planes == 3))
    assert info["path"] == FUSED and info["tiles"][:2] == (256, 128)
    assert info["names"] == info["names32"] and not any(n.startswith("convert") for n in info["names"]), info["names"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,shape", [(64, (3 * 64 + 20, 3 * 256 + 8)), (32, (5 * 32, 2 * 256))], ids=["rows64", "rows32"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
def test_native_2d_other_tile_heights(kind, rows, shape, clamped):
    scans = rc.xy_pm(rc.GAUSS2)
    info = _both(shape, scans, clamped, [rc.random_image(shape, np.float32, 71)], kind, flags=TILED | capi.RF_PLAN_TILE_ROWS(rows))
    assert info["path"] == FUSED and info["tiles"][1] == rows
    assert info["names"] == info["names32"] and not any(n.startswith("convert") for n in info["names"]), info["names"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flag", ["RF_PLAN_FULL_CARRY_SCAN", "RF_PLAN_MFMA_PASS1", "RF_PLAN_STAGED_PASS1"])
def test_native_2d_plan_options(kind, flag):
    """the full carry scans, and both pass-1 kernels reading 16-bit planes"""
    shape, scans = (4 * 128, 6 * 256), rc.xy_pm(rc.GAUSS2)
    info = _both(shape, scans, True, [rc.random_image(shape, np.float32, 72)], kind,
                 flags=TILED | capi.RF_PLAN_TILE_ROWS(128) | getattr(capi, flag))
    assert info["path"] == FUSED and info["names"] == info["names32"], info["names"]
    assert ("carry_y" in info["names"]) == (flag == "RF_PLAN_FULL_CARRY_SCAN")


# ---- exactness -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(256, 512), (200, 516)], ids=["whole_tiles", "partial_tiles"])
def test_summed_area_table_is_exact(kind, shape):
    """Integers 0..3 are exact in both types and every partial sum stays below 2^24, so the f32 result is exact in any
    summation order: the output is torch's rounding of the exact table, bit for bit -- +inf above 65504 in binary16 included."""
    import torch
    tdt = _types()[kind][0]
    img = np.random.default_rng(73).integers(0, 4, size=shape).astype(np.float32)
    scans = [(0, True, [1.0, 1.0]), (1, True, [1.0, 1.0])]
    got, names, path, _, _ = _run(shape, scans, False, [_narrow(img, kind)], tdt)
    exact = np.cumsum(np.cumsum(img.astype(np.float64), axis=0), axis=1)
    assert exact.max() < 2 ** 24
    want = torch.from_numpy(exact.astype(np.float32)).to(tdt)
    assert path == FUSED and not any(n.startswith("convert") for n in names)
    assert torch.equal(_bits(got[0]), _bits(want))
    if kind == "f16":
        assert bool(torch.isinf(got[0]).any())


# ---- pointwise stages ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", [128, 64])
def test_pointwise_stages_native(kind, rows):
    """prologue (1/255, 0) and an unsharp-mask epilogue, both in f32 before the single rounding"""
    shape, scans = (2 * 128 + 64, 4 * 256), rc.xy_pm(rc.GAUSS2)
    img = np.floor(rc.random_image(shape, np.float32, 74) * 255.0).astype(np.float32)      # (integers up to 255: exact in both types)
    info = _both(shape, scans, True, [img], kind, flags=TILED | capi.RF_PLAN_TILE_ROWS(rows), oracle_check=False,
                 prologue=(1.0 / 255.0, 0.0), epilogue=(-0.5, 1.5, 1.0))       # (stays above 0.5)
    assert info["path"] == FUSED and info["names"] == info["names32"], info["names"]


# ---- 1-D -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_signal_biquad_pair_native(kind):
    n, scans = 16 * 8192, [(0, True, rc.GAUSS2), (0, False, rc.GAUSS2)]
    info = _both((n,), scans, False, [rc.random_image((n,), np.float32, 75)], kind)
    assert info["path"] == FUSED and not any(n_.startswith("convert") for n_ in info["names"]), info["names"]
    assert info["names"] == info["names32"]


@pytest.mark.parametrize("kind", KINDS)
def test_signal_ragged_length(kind):
    """a causal biquad over a length that ends inside a chunk: the samples at the signal's end are loaded one by one"""
    n, scans = 100003, [(0, True, rc.GAUSS2)]
    _both((n,), scans, False, [rc.random_image((n,), np.float32, 76)], kind)


# ---- staged ----------------------------------------------------------------------------------------------------------
def _staged_checks(info, planes, samples):
    if any(n.startswith("convert") for n in info["names"]):
        assert info["names"][0] == "convert_in" and info["names"][-1] == "convert_out", info["names"]
        assert info["names"][1:-1] == info["names32"], (info["names"], info["names32"])
        assert info["ws"] >= planes * samples * 4
        assert info["path"] == info["path32"]
        return True
    return False


@pytest.mark.parametrize("kind", KINDS)
def test_staged_volume(kind):
    shape = (64, 96, 128)
    scans = rc.xy_pm(rc.GAUSS2) + [(2, True, rc.GAUSS2), (2, False, rc.GAUSS2)]
    info = _both(shape, scans, True, [rc.random_image(shape, np.float32, 77)], kind, path=AUTO)
    assert _staged_checks(info, 1, int(np.prod(shape)))


@pytest.mark.parametrize("kind", KINDS)
def test_staged_order_5_clamped(kind):
    shape = (256, 512)
    w = [0.5, 0.1, 0.1, 0.1, 0.1, 0.1]       # (positive impulse response, unit gain: positive results)
    scans = rc.xy_pm(w)
    info = _both(shape, scans, True, [rc.random_image(shape, np.float32, 78) + np.float32(1.0)], kind, path=AUTO)
    assert _staged_checks(info, 1, int(np.prod(shape)))


@pytest.mark.parametrize("kind", KINDS)
def test_staged_odd_width(kind):
    shape = (300, 1001)
    info = _both(shape, rc.xy_pm(rc.GAUSS2), True, [rc.random_image(shape, np.float32, 79)], kind, path=AUTO)
    assert _staged_checks(info, 1, int(np.prod(shape)))


@pytest.mark.parametrize("kind", KINDS)
def test_small_image_on_the_shipped_defaults(kind, shipped_defaults):
    """RF_PATH_AUTO with flags = 0: whichever form the plan picks keeps the one-rounding contract"""
    shape = (200, 300)
    info = _both(shape, rc.xy_pm(rc.GAUSS2), True, [rc.random_image(shape, np.float32, 80)], kind, path=AUTO, flags=0)
    _staged_checks(info, 1, int(np.prod(shape)))


@pytest.mark.parametrize("kind", KINDS)
def test_stage_half_flag_gives_the_staged_form(kind):
    shape = (2 * 128, 3 * 256)
    info = _both(shape, rc.xy_pm(rc.GAUSS2), True, [rc.random_image(shape, np.float32, 81)] * 2, kind, path=AUTO,
                 flags=TILED | capi.RF_PLAN_STAGE_HALF)
    assert _staged_checks(info, 2, int(np.prod(shape)))


# ---- sharded ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_rank_through_the_stepping_calls(kind):
    import torch
    import recfilter_amd as rfa
    tdt = _types()[kind][0]
    shape, scans = (4 * 64, 3 * 256), rc.xy_pm(rc.GAUSS2)
    x = _narrow(rc.random_image(shape, np.float32, 82), kind)
    whole, _, _, _, _ = _run(shape, scans, True, [x], tdt)
    with rfa.Plan(shape, scans, dtype=tdt, clamped=True, path=FUSED, flags=TILED | capi.RF_PLAN_FORCE_EXCHANGE) as plan:
        dev, out = x.cuda(), torch.empty(shape, dtype=tdt, device="cuda")
        assert plan.path == FUSED and plan.num_exchanges >= 1
        plan.begin([dev], [out])
        for i in range(plan.num_exchanges):
            send = torch.zeros(plan.exchange_bytes(i), dtype=torch.uint8, device="cuda")
            plan.exchange_local(i, send.data_ptr())
            plan.exchange_apply(i, send.data_ptr())       # the all-gather of one rank is the identity
        plan.finish()
        torch.cuda.synchronize()
        got = out.cpu()
    d = (_bits(got) - _bits(whole[0])).abs()
    assert int(d.max()) <= 1 and float((d == 0).double().mean()) >= 0.98


# ---- full size -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_cfg3_16384_against_the_f32_plan(kind):
    """the headline configuration: three launches, assertion 2 (tests/test_gpu_fullsize.py pins the f32 plan to the oracle)"""
    import torch
    import recfilter_amd as rfa
    c = rc.BASELINE_CONFIGS["cfg3_gaussian2_xy"]
    tdt = _types()[kind][0]
    x16 = rc.cuda_image(c["shape"], np.float32, 9).to(tdt)
    with rfa.Plan(c["shape"], c["scans"], dtype=tdt, clamped=c["clamped"], path=FUSED, flags=0) as p16:
        got, timed = p16.execute_timed([x16])
        names = [n for n, _ in timed]
    with rfa.Plan(c["shape"], c["scans"], dtype=torch.float32, clamped=c["clamped"], path=FUSED, flags=0) as p32:
        ref, timed32 = p32.execute_timed([x16.float()])
    assert names == ["fused_tails", "xscan_rows", "fused_pass2"] == [n for n, _ in timed32], names
    ref16 = ref[0].to(tdt)
    assert bool((ref[0] > 0).all())
    d = (got[0].view(torch.int16).to(torch.int32) - ref16.view(torch.int16).to(torch.int32)).abs()
    worst, same = int(d.max()), float((d == 0).double().mean())
    print(f"cfg3 {kind}: max bit difference {worst}, identical {100.0 * same:.4f} %")
    assert worst <= 1 and same >= 0.98


# ---- C++ front end ---------------------------------------------------------------------------------------------------
def test_cpp_frontend_half(tmp_path):
    """RecFilterImage(const rf_half *) through realize() on a 512 x 512 Gaussian, against the raster loops of the existing C++
    test at 1e-4 + 2^-11; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_half.cpp")
    exe = str(tmp_path / "test_frontend_half")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "half-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
