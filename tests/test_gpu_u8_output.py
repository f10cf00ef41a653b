"""Byte planes on both sides (rf_input_dtype RF_IO_U8) on the GPU: out = sat8(F_f32(widen(in))), converted once at the final
store.  The per-sample rule, its derivation and the shapes are in tests/u8_cases.py; tests/test_u8_output_host.py shows that a
correct f32 implementation passes the rule on these very inputs.

Native plans (2-D images whose width is a multiple of 4, on the fused kernels) list the RF_IN_U8 plan's launches; staged plans
(everything else) list them plus a trailing convert_out."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import ref_cases as rc
import u8_cases as u8
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

TILED = capi.RF_PLAN_TILED_ONLY
FUSED = capi.RF_PATH_TILED_FUSED
AUTO = capi.RF_PATH_AUTO
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IO = dict(dtype=np.float32, input_dtype=np.uint8, output_dtype=np.uint8)
IN = dict(dtype=np.float32, input_dtype=np.uint8)


def _run(shape, scans, clamped, imgs, flags, path=AUTO, inplace=False, bytes_out=True, **kw):
    """imgs: host uint8 arrays.  Returns (outputs as host numpy arrays, launch names, path, workspace bytes)."""
    import torch
    import recfilter_amd as rfa
    with rfa.Plan(shape, scans, clamped=clamped, planes=len(imgs), path=path, flags=flags, **(IO if bytes_out else IN), **kw) as plan:
        dev = [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]
        if inplace:
            _, timed = plan.execute_timed(dev, dev)
            outs = dev
        else:
            outs, timed = plan.execute_timed(dev)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs], [n for n, _ in timed], plan.path, plan.workspace_bytes


def _assert_rule(got, img, scans, clamped, prologue=None, epilogue=None, what=""):
    want, scale = u8.want_and_scale(img, scans, clamped, prologue, epilogue)
    excess = u8.rule_excess(got, want, scale)
    print(f"{what}: worst |got - clip(want)| - (0.5 + 1e-4 scale) = {excess:.4e}")
    assert got.dtype == np.uint8
    assert excess <= 0.0


# ---- exact cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,flags,name", u8.NATIVE_SHAPES, ids=u8.NATIVE_IDS)
def test_identity_is_exact(shape, flags, name):
    img = u8.byte_image(shape, u8.seed_of(shape))
    got, names, path, _ = _run(shape, [(0, True, [1.0, 0.0])], False, [img], TILED | flags)
    assert path == FUSED and not any(n.startswith("convert") for n in names), names
    assert np.array_equal(got[0], img)


TABLE_SHAPE = (200, 516)
TABLE_SCANS = [(0, True, [1.0, 1.0]), (1, True, [1.0, 1.0])]


@pytest.fixture(scope="module")
def table():
    """bytes from {0,1,2,3} and their exact summed-area table: every partial sum stays below 2^24, so the f32 table is exact
    in any summation order"""
    img = np.random.default_rng(9101).integers(0, 4, size=TABLE_SHAPE).astype(np.uint8)
    exact = np.cumsum(np.cumsum(img.astype(np.float64), axis=0), axis=1)
    assert exact.max() < 2 ** 24 and exact.max() > 512 * 100
    exact.setflags(write=False)
    return img, exact


@pytest.mark.parametrize("epilogue,name", [(None, "saturating"), ((2.0 ** -10, 0.0, 0.0), "ties"), ((2.0 ** -9, 0.0, 0.0), "ties_saturating"),
                                           ((-1.0, 0.0, 10.0), "negative")],
                         ids=["saturating", "ties", "ties_saturating", "negative"])
def test_summed_area_table_is_exact(table, epilogue, name):
    """bit for bit against clip(rint(v), 0, 255) of the exact v.  (2^-10: ties at the odd multiples of 512 decide half-to-even;
    this table's far corner, about 155,000, stays at 151 under it, so 2^-9 runs as well: ties AND a saturating corner.)"""
    img, exact = table
    v = exact if epilogue is None else epilogue[0] * exact + epilogue[2]         # exact in f32: a power of two / small integers
    want = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    got, names, path, _ = _run(TABLE_SHAPE, TABLE_SCANS, False, [img], TILED, epilogue=epilogue)
    assert path == FUSED and not any(n.startswith("convert") for n in names), names
    if name == "saturating":
        assert want[-1, -1] == 255 and np.array_equal(want, np.minimum(exact, 255).astype(np.uint8))
    if name == "ties":
        assert np.any(np.mod(exact, 1024) == 512)                               # ties happen
    if name == "ties_saturating":
        assert np.any(np.mod(exact, 512) == 256) and want[-1, -1] == 255        # ... and here the far corner saturates too
    if name == "negative":
        assert v.min() < 0 and want.min() == 0 and want.max() == 10 - int(img[0, 0]) and (want == 0).mean() > 0.9      # (the largest value is the first sample's)
    assert np.array_equal(got[0], want)


# ---- the one-rounding rule ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(shape, plane=0):
        key = (tuple(shape), plane)
        if key not in cache:
            cache[key] = u8.byte_image(shape, u8.seed_of(shape, plane))
            cache[key].setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("case", u8.GAUSS_CASES, ids=u8.GAUSS_IDS)
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("setup", u8.SETUPS, ids=u8.SETUP_IDS)
@pytest.mark.parametrize("planes", [1, 3])
def test_gaussians_round_once(inputs, case, clamped, setup, planes):
    (shape, flags, name), scans = u8.NATIVE_SHAPES[case[0]], rc.xy_pm(getattr(rc, case[1]))
    _, prologue, epilogue = setup
    inplace = planes == 3 and not (epilogue is not None and epilogue[1] != 0.0)     # (an input operand needs out != in)
    imgs = [inputs(shape, p) for p in range(planes)]
    kw = dict(prologue=prologue, epilogue=epilogue)
    got, names, path, ws = _run(shape, scans, clamped, imgs, TILED | flags, inplace=inplace, **kw)
    ref, names_in, path_in, ws_in = _run(shape, scans, clamped, imgs, TILED | flags, bytes_out=False, **kw)
    assert path == FUSED and path_in == FUSED
    assert names == names_in and not any(n.startswith("convert") for n in names), (names, names_in)
    assert ws == ws_in
    for p in range(planes):
        _assert_rule(got[p], imgs[p], scans, clamped, prologue, epilogue, f"{name} plane {p}")
        d = np.abs(got[p].astype(np.int32) - u8.sat8(ref[p]).astype(np.int32))
        print(f"{name} plane {p}: against sat8 of the RF_IN_U8 plan: max byte difference {int(d.max())}, identical {100.0 * float((d == 0).mean()):.4f} %")
        assert int(d.max()) <= 1


# ---- staged ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scans,name", u8.STAGED_SHAPES, ids=[s[2] for s in u8.STAGED_SHAPES])
def test_staged_shapes(shape, scans, name):
    clamped = name == "odd_width"
    img = u8.byte_image(shape, u8.seed_of(shape))
    got, names, path, ws = _run(shape, scans, clamped, [img], TILED)
    _, names_in, path_in, ws_in = _run(shape, scans, clamped, [img], TILED, bytes_out=False)
    assert names == names_in + ["convert_out"], (names, names_in)
    assert path == path_in and ws >= ws_in + int(np.prod(shape)) * 4
    _assert_rule(got[0], img, scans, clamped, what=name)


def test_stage_half_flag_gives_the_staged_form(inputs):
    shape, flags, name = u8.NATIVE_SHAPES[0]
    scans, img = rc.xy_pm(rc.GAUSS2), inputs(shape)
    got, names, path, ws = _run(shape, scans, True, [img], TILED | flags | capi.RF_PLAN_STAGE_HALF)
    native, names_native, _, _ = _run(shape, scans, True, [img], TILED | flags)
    assert names == names_native + ["convert_out"] and path == FUSED, names
    _assert_rule(got[0], img, scans, True, what="staged by flag")
    assert int(np.abs(got[0].astype(np.int32) - native[0].astype(np.int32)).max()) <= 1


# ---- footprint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,flags,name", [u8.NATIVE_SHAPES[0], u8.NATIVE_SHAPES[1], ((64, 250), 0, "staged_odd_width")],
                         ids=["partial_rows_tall", "last_column_4_wide", "staged_odd_width"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_footprint_and_statelessness(shape, flags, name, inplace):
    import torch
    import recfilter_amd as rfa
    scans, planes = rc.xy_pm(rc.GAUSS2), 2
    A = [torch.from_numpy(u8.byte_image(shape, u8.seed_of(shape, p))) for p in range(planes)]
    poison = [torch.full(shape, 255, dtype=torch.uint8) for _ in range(planes)]
    mk = lambda: rfa.Plan(shape, scans, clamped=True, planes=planes, flags=TILED | flags, **IO)
    with mk() as plan:
        run = lambda ins, outs: plan.execute(ins, outs)
        results = [guarded.guarded_execute(run, shape, np.uint8, np.uint8, A, inplace=inplace, in_fill=fill)
                   for fill in (guarded.IN_FILL, guarded.IN_FILL_ZERO)]
        guarded.assert_bits_equal(results[0], results[1], "0xFF against 0x00 input guards (a load past a plane)")
        r1 = guarded.three_steps(plan, A, poison, out_dtype=np.uint8, inplace=inplace)
        guarded.assert_bits_equal(results[0], r1, "guarded planes against plain planes")
    with mk() as fresh:
        guarded.poisoned_scratch(fresh, A, r1, out_dtype=np.uint8, inplace=inplace)
    for p in range(planes):
        _assert_rule(r1[p].numpy(), A[p].numpy(), scans, True, what=f"{name} plane {p}")


# ---- front ends ------------------------------------------------------------------------------------------------------------
def test_python_frontend_to_bytes():
    import torch
    from recfilter_amd.filter import RecFilter, RecFilterDim, Pointwise
    shape, scans = (2 * 128 + 70, 5 * 256), rc.xy_pm(rc.GAUSS2)
    img = u8.byte_image(shape, u8.seed_of(shape))
    x, y = RecFilterDim("x", shape[1]), RecFilterDim("y", shape[0])
    f = RecFilter("Blur8")
    f.set_clamped_image_border()
    f.define([x, y], torch.from_numpy(img).cuda(), scale=1.0 / 255.0)
    for dim, causal, coeff in scans:
        f.add_filter(+[x, y][dim] if causal else -[x, y][dim], coeff)
    f.compute_at(Pointwise(255.0, to_bytes=True))
    f.compile_jit(path=FUSED)
    out = f.realize()[0]
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == shape
    _assert_rule(out.cpu().numpy(), img, scans, True, (1.0 / 255.0, 0.0), (255.0, 0.0, 0.0), "python front end")


def test_float_output_tensor_is_a_type_error():
    import torch
    import recfilter_amd as rfa
    shape = (64, 256)
    with rfa.Plan(shape, rc.xy_pm(rc.GAUSS2), clamped=True, flags=TILED, **IO) as plan:
        src = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        with pytest.raises(TypeError):
            plan.execute([src], [torch.empty(shape, dtype=torch.float32, device="cuda")])
        assert plan.execute([src])[0].dtype == torch.uint8


def test_cpp_frontend_u8(tmp_path):
    """RecFilterImage(const uint8_t *) with a to_bytes consumer through realize() on a 512 x 512 Gaussian, against the raster
    loops of the existing C++ test under the one-rounding rule; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_u8.cpp")
    exe = str(tmp_path / "test_frontend_u8")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "u8-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
