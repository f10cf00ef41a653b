"""Byte volumes (rf_input_dtype RF_IO_U8, three dimensions) on the GPU: out = sat8(post_f * F_f32(widen(in)) + post_b),
converted once, by the final z pass (strided_final_u8_kernel).  The per-sample rule and its derivation are in tests/u8_cases.py;
tests/test_u8_volumes_host.py shows that a correct f32 implementation passes it on these very inputs.

A native plan lists the launches of the RF_IN_U8 plan with two first passes (RF_PLAN_STAGED_PASS1) without its stand-alone
pointwise_post, has no convert_* step and owns one f32 volume per plane more; a staged plan lists a trailing convert_out."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import ref_cases as rc
import u8_cases as u8
import u8_volume_cases as vc
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

TILED, FUSED, AUTO, IO, IN = vc.TILED, vc.FUSED, vc.AUTO, vc.IO, vc.IN
TWO_PASSES = capi.RF_PLAN_STAGED_PASS1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [(0, True, [1.0, 0.0]), (1, True, [1.0, 0.0]), (2, True, [1.0, 0.0])]


def _run(shape, scans, clamped, imgs, flags=TILED, path=FUSED, inplace=False, bytes_out=True, **kw):
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


def _assert_native(names, path, ws, names_in, ws_in, shape, planes):
    """the launch list of the RF_IN_U8 plan with two first passes, minus pointwise_post; no conversion step; the f32 volumes"""
    assert path == FUSED
    assert not any(n.startswith("convert") for n in names), names
    assert names == [n for n in names_in if n != "pointwise_post"], (names, names_in)
    assert names[-1] == "strided_pass2_z", names
    assert ws >= ws_in + 4 * int(np.prod(shape)) * planes


def _assert_rule(got, img, scans, clamped, prologue=None, epilogue=None, what="", wants=None, key=None):
    if wants is not None and key in wants:
        want, scale = wants.pop(key)
    else:
        want, scale = u8.want_and_scale(img, scans, clamped, prologue, epilogue)
        if wants is not None and key[1] == 0:
            wants.clear()
            wants[key] = (want, scale)
    excess = u8.rule_excess(got, want, scale)
    print(f"{what}: worst |got - clip(want)| - (0.5 + 1e-4 scale) = {excess:.4e}")
    assert got.dtype == np.uint8
    assert excess <= 0.0


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


@pytest.fixture(scope="module")
def wants():
    """(want, scale) of the f64 oracle for plane 0 of the case last run, keyed (shape, plane, scans, border, setup): computed once,
    shared by the one-plane and the three-plane run of a case (plane 0 is the same image), read only, dropped after the second"""
    return {}


# ---- exact cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 96, 128), (96, 200, 260)], ids=str)
def test_identity_is_exact(inputs, shape):
    img = inputs(shape)
    got, names, path, ws = _run(shape, IDENTITY, False, [img])
    _, names_in, _, ws_in = _run(shape, IDENTITY, False, [img], flags=TILED | TWO_PASSES, bytes_out=False)
    _assert_native(names, path, ws, names_in, ws_in, shape, 1)
    assert np.array_equal(got[0], img)


TABLE_SHAPE = (32, 64, 256)
TABLE_SCANS = [(0, True, [1.0, 1.0]), (1, True, [1.0, 1.0]), (2, True, [1.0, 1.0])]


@pytest.fixture(scope="module")
def table():
    """bytes from {0, 1} and their exact summed-volume table: every partial sum stays below 2^24 (the volume has 2^19 samples),
    so the f32 table is exact in any summation order"""
    img = np.random.default_rng(9102).integers(0, 2, size=TABLE_SHAPE).astype(np.uint8)
    exact = np.cumsum(np.cumsum(np.cumsum(img.astype(np.float64), axis=0), axis=1), axis=2)
    assert exact.max() < 2 ** 24 and exact.max() > 200000
    exact.setflags(write=False)
    return img, exact


@pytest.mark.parametrize("epilogue,name", [(None, "saturating"), ((2.0 ** -11, 0.0, 0.0), "ties"), ((-(2.0 ** -4), 0.0, 100.0), "negative")],
                         ids=["saturating", "ties", "negative"])
def test_summed_volume_table_is_exact(table, epilogue, name):
    """bit for bit against clip(rint(v), 0, 255) of the exact v.  2^-11: the far corner, about 262,000, is about 128, and the ties
    at the odd multiples of 1024 decide half-to-even.  -(2^-4) v + 100: exact in f32 (a power of two, a small integer), below zero
    for most of the volume."""
    img, exact = table
    v = exact if epilogue is None else epilogue[0] * exact + epilogue[2]
    want = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    got, names, path, _ = _run(TABLE_SHAPE, TABLE_SCANS, False, [img], epilogue=epilogue)
    assert path == FUSED and not any(n.startswith("convert") or n == "pointwise_post" for n in names), names
    if name == "saturating":
        assert want[-1, -1, -1] == 255 and np.array_equal(want, np.minimum(exact, 255).astype(np.uint8))
    if name == "ties":
        assert np.any(np.mod(exact, 2048) == 1024) and want.max() > 100                 # ties happen
    if name == "negative":
        assert v.min() < 0 and want.min() == 0 and want.max() >= 99 and (want == 0).mean() > 0.5
    assert np.array_equal(got[0], want)


# ---- the one-rounding rule ---------------------------------------------------------------------------------------------
def _round_once(inputs, shape, scans, clamped, setup, planes, flags=TILED, what="", wants=None):
    _, prologue, epilogue = setup
    imgs = [inputs(shape, p) for p in range(planes)]
    kw = dict(prologue=prologue, epilogue=epilogue)
    got, names, path, ws = _run(shape, scans, clamped, imgs, flags=flags, inplace=planes == 3, **kw)
    ref, names_in, path_in, ws_in = _run(shape, scans, clamped, imgs, flags=flags | TWO_PASSES, bytes_out=False, **kw)
    assert path_in == FUSED
    _assert_native(names, path, ws, names_in, ws_in, shape, planes)
    for p in range(planes):
        _assert_rule(got[p], imgs[p], scans, clamped, prologue, epilogue, f"{what} plane {p}", wants,
                     (tuple(shape), p, repr(scans), clamped, setup[0]))
        d = np.abs(got[p].astype(np.int32) - u8.sat8(ref[p]).astype(np.int32))
        print(f"{what} plane {p}: against sat8 of the RF_IN_U8 plan: max byte difference {int(d.max())}, identical {100.0 * float((d == 0).mean()):.4f} %")
        assert int(d.max()) <= 1
    return names


# The grid in full: 3 shapes x 3 z patterns x 2 filters x 2 borders x 4 setups x (one plane out of place, three planes in place).
# (the plane count varies fastest: the two runs of a case follow each other and share plane 0's oracle result)
@pytest.mark.parametrize("planes", [1, 3], ids=["one_plane", "three_planes_in_place"])
@pytest.mark.parametrize("setup", vc.SETUPS, ids=vc.SETUP_IDS)
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3"])
@pytest.mark.parametrize("zpat", vc.Z_PATTERNS)
@pytest.mark.parametrize("shape", vc.GPU_SHAPES, ids=str)
def test_gaussians_round_once(inputs, wants, planes, shape, zpat, coeff, clamped, setup):
    _round_once(inputs, shape, vc.scans_of(getattr(rc, coeff), zpat), clamped, setup, planes, wants=wants,
                what=f"{shape} {zpat} {coeff} {'clamped' if clamped else 'zero'} {setup[0]}")


@pytest.mark.parametrize("planes_tile", [32, 64, 128])
@pytest.mark.parametrize("zpat", ["pair", "causal"])
def test_z_tile_widths(inputs, planes_tile, zpat):
    """32, 64 and 128 planes per thread (RF_PLAN_TILE_PLANES), on the uniform instances of both scan patterns"""
    shape = (256, 64, 256)
    _round_once(inputs, shape, vc.scans_of(rc.GAUSS2, zpat), True, vc.SETUPS[2], 1, flags=TILED | capi.RF_PLAN_TILE_PLANES(planes_tile),
                what=f"z tile {planes_tile} {zpat}")


@pytest.mark.parametrize("planes_tile", [32, 128])
def test_z_tile_widths_general_instance(inputs, planes_tile):
    """the general instance (lines no multiple of 256) at the smallest and the largest tile: (128, 40, 132)"""
    shape = (128, 40, 132)
    _round_once(inputs, shape, vc.scans_of(rc.GAUSS3, "pair"), False, vc.SETUPS[0], 1, flags=TILED | capi.RF_PLAN_TILE_PLANES(planes_tile),
                what=f"general, z tile {planes_tile}")


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("shape", [(64, 96, 128), (96, 200, 260)], ids=str)
def test_orders(inputs, order, shape):
    coeff = {1: vc.ORDER1, 2: rc.GAUSS2, 3: rc.GAUSS3}[order]
    _round_once(inputs, shape, vc.scans_of(coeff, "pair"), True, vc.SETUPS[0], 1, what=f"order {order} {shape}")


def test_mixed_z_scans_take_the_general_pattern(inputs):
    """anticausal then causal along z, and x scans alone in front: no usual pattern"""
    shape = (64, 96, 128)
    scans = [(0, True, rc.GAUSS2), (0, False, rc.GAUSS2), (2, False, rc.GAUSS2), (2, True, rc.GAUSS2)]
    _round_once(inputs, shape, scans, True, vc.SETUPS[0], 1, what="x and -z +z")


# ---- staged ------------------------------------------------------------------------------------------------------------
def test_stage_half_flag_gives_the_staged_form(inputs):
    shape, scans, img = (64, 96, 128), vc.scans_of(rc.GAUSS2, "pair"), inputs((64, 96, 128))
    got, names, path, ws = _run(shape, scans, True, [img], flags=TILED | capi.RF_PLAN_STAGE_HALF)
    native, names_native, _, _ = _run(shape, scans, True, [img])
    _, names_in, _, _ = _run(shape, scans, True, [img], bytes_out=False)
    assert names == names_in + ["convert_out"] and not any(n.startswith("convert") for n in names_native), (names, names_native)
    _assert_rule(got[0], img, scans, True, what="staged by flag")
    assert int(np.abs(got[0].astype(np.int32) - native[0].astype(np.int32)).max()) <= 1


def test_small_volume_on_the_automatic_path_is_staged(inputs):
    shape, scans, img = (64, 96, 128), vc.scans_of(rc.GAUSS2, "pair"), inputs((64, 96, 128))
    got, names, _, _ = _run(shape, scans, True, [img], path=AUTO)
    assert names[-1] == "convert_out", names
    _assert_rule(got[0], img, scans, True, what="automatic path, small")


# ---- footprint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 96, 128), (96, 200, 260)], ids=str)
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_footprint_and_statelessness(shape, inplace):
    import torch
    import recfilter_amd as rfa
    scans, planes = vc.scans_of(rc.GAUSS2, "pair"), 2
    A = [torch.from_numpy(u8.byte_image(shape, u8.seed_of(shape, p))) for p in range(planes)]
    poison = [torch.full(shape, 255, dtype=torch.uint8) for _ in range(planes)]
    mk = lambda: rfa.Plan(shape, scans, clamped=True, planes=planes, path=FUSED, flags=TILED, epilogue=(0.5, 0.0, 16.0), **IO)
    with mk() as plan:
        run = lambda ins, outs: plan.execute(ins, outs)
        results = [guarded.guarded_execute(run, shape, np.uint8, np.uint8, A, inplace=inplace, in_fill=fill)
                   for fill in (guarded.IN_FILL, guarded.IN_FILL_ZERO)]
        guarded.assert_bits_equal(results[0], results[1], "0xFF against 0x00 input guards (a load past a plane)")
        r1 = guarded.three_steps(plan, A, poison, out_dtype=np.uint8, inplace=inplace)
        guarded.assert_bits_equal(results[0], r1, "guarded planes against plain planes")
    with mk() as fresh:
        assert guarded.poisoned_scratch(fresh, A, r1, out_dtype=np.uint8, inplace=inplace) >= planes      # (the f32 volumes among them)
    for p in range(planes):
        _assert_rule(r1[p].numpy(), A[p].numpy(), scans, True, None, (0.5, 0.0, 16.0), what=f"{shape} plane {p}")


# ---- front ends ------------------------------------------------------------------------------------------------------------
def test_python_frontend_to_bytes_volume():
    import torch
    import recfilter_amd as rfa
    from recfilter_amd.filter import RecFilter, RecFilterDim, Pointwise
    shape, scans = (64, 96, 128), vc.scans_of(rc.GAUSS2, "pair")
    img = u8.byte_image(shape, u8.seed_of(shape))
    dims = [RecFilterDim("x", shape[2]), RecFilterDim("y", shape[1]), RecFilterDim("z", shape[0])]
    f = RecFilter("Blur8Volume")
    f.set_clamped_image_border()
    f.define(dims, torch.from_numpy(img).cuda(), scale=1.0 / 255.0)
    for dim, causal, coeff in scans:
        f.add_filter(+dims[dim] if causal else -dims[dim], coeff)
    f.compute_at(Pointwise(255.0, to_bytes=True))
    f.compile_jit(path=FUSED)
    plan = f._contents["plan"]
    with rfa.Plan(shape, scans, clamped=True, path=FUSED, prologue=(1.0 / 255.0, 0.0), epilogue=(255.0, 0.0, 0.0), **IN) as pin:
        assert plan.path == FUSED and plan.num_kernels == pin.num_kernels - 1        # native: no convert_out, no pointwise_post
        assert plan.workspace_bytes >= pin.workspace_bytes + 4 * int(np.prod(shape))
    out = f.realize()[0]
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == shape
    _assert_rule(out.cpu().numpy(), img, scans, True, (1.0 / 255.0, 0.0), (255.0, 0.0, 0.0), "python front end")


def test_cpp_frontend_u8_volume(tmp_path):
    """RecFilterImage(const uint8_t *) with a to_bytes consumer through realize(), against raster loops under the one-rounding
    rule, on two Gaussians: 64 x 128 x 256 (2^21 samples), which must run the NATIVE plan -- the program compares launches and
    workspace with the RF_IN_U8 plan's through RecFilter::plan() and fails where the final z pass does not store the bytes -- and
    64 x 96 x 256, below the threshold of RF_PATH_AUTO (the only path the C++ front end asks for), which must run the staged one.
    Compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_u8_volume.cpp")
    exe = str(tmp_path / "test_frontend_u8_volume")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "u8-volume-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
