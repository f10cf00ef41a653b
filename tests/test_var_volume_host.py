"""CPU tests of the varying scans and the smoothing plan on volumes (rf_var_plan_create_volume, rf_smooth_plan_create_volume,
rf_var_distances_volume): host-only plans -- the accepted domain on both sides of each limit, every refusal with its status and a
message that names the limit, the exact workspace, launch counts and names -- and the loops of tests/var_volume_loops.py, the
yardstick of the GPU tests, pinned by central differences in f64.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import recfilter_amd as rfa
import var_volume_loops as vloops
from recfilter_amd import capi

PX, MX, PY, MY, PZ, MZ = (0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1), (2, True, 2), (2, False, 2)
SCAN_LISTS = {"+z": [PZ], "-z": [MZ], "+z-z": [PZ, MZ], "-z+z": [MZ, PZ], "+x-x+y-y+z-z": [PX, MX, PY, MY, PZ, MZ],
              "+z-z two weights": [(2, True, 2), (2, False, 1)], "+x-x": [PX, MX], "+y": [PY]}
STAGES = {"+z": 1, "-z": 1, "+z-z": 1, "-z+z": 2, "+x-x+y-y+z-z": 3, "+z-z two weights": 2, "+x-x": 1, "+y": 1}
HOST = capi.RF_DEVICE_HOST_ONLY


def host_plan(shape, scans, planes=1, n_weights=3):
    return rfa.VarPlan.volume(shape, scans, planes=planes, n_weights=n_weights, device=HOST)


def raw_create(edit, scans=((2, 1, 0),)):
    """rf_var_plan_create_volume on a valid host-only description of 64 x 40 x 8 after edit(desc); returns (status, message)"""
    arr = (capi.VarScanDesc * len(scans))()
    for i, (dim, causal, weights) in enumerate(scans):
        arr[i].dim, arr[i].causal, arr[i].weights = dim, causal, weights
    d = capi.VarVolumeDesc()
    d.abi, d.width, d.height, d.depth, d.dtype = capi.RF_ABI, 64, 40, 8, capi.RF_F32
    d.n_planes, d.n_weights = 1, 1
    d.n_scans, d.scans = len(scans), ctypes.cast(arr, ctypes.POINTER(capi.VarScanDesc))
    d.device, d.flags = HOST, 0
    edit(d)
    h = ctypes.c_void_p()
    status = capi.lib().rf_var_plan_create_volume(ctypes.byref(d), ctypes.byref(h))
    message = capi.lib().rf_last_error_string().decode()
    if status == capi.RF_OK:
        capi.lib().rf_var_plan_destroy(h)
    else:
        assert not h.value, "a refused description must not leave a plan behind"
    return status, message


def fields(**values):
    def edit(d):
        for name, value in values.items():
            setattr(d, name, value)
    return edit


# ---- the accepted domain --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planes", [
    ((512, 512, 512), 1), ((64, 2048, 2048), 1),              # the second: 2^22 z lines, above the 2-D extent cap
    ((1, 1, 4), 1), ((1, 1, 1 << 21), 1), ((1, 1 << 21, 4), 1), ((65535, 1, 4), 1),
    ((1, 1 << 15, 1 << 15), 1),                                # width * height = 2^30
    ((4095, 8, 8), 16), ((21845, 8, 8), 3),                    # depth * planes = 65520, 65535
])
def test_valid_volume_is_accepted(shape, planes):
    D, H, W = shape
    status, message = raw_create(fields(depth=D, height=H, width=W, n_planes=planes))
    assert status == capi.RF_OK, message


@pytest.mark.parametrize("what,edit,scans,status,text", [
    ("width 6", fields(width=6), None, capi.RF_ERR_UNSUPPORTED, "multiple of 4"),
    ("width 66", fields(width=66), None, capi.RF_ERR_UNSUPPORTED, "multiple of 4"),
    ("width 2^21 + 4", fields(width=(1 << 21) + 4, height=1), None, capi.RF_ERR_UNSUPPORTED, str(1 << 21)),
    ("height 2^21 + 1", fields(height=(1 << 21) + 1, width=4), None, capi.RF_ERR_UNSUPPORTED, str(1 << 21)),
    ("depth 2^21 + 1", fields(depth=(1 << 21) + 1), None, capi.RF_ERR_UNSUPPORTED, str(1 << 21)),
    ("width * height 2^30 + 2^15", fields(width=1 << 15, height=(1 << 15) + 1, depth=1), None, capi.RF_ERR_UNSUPPORTED, "width * height"),
    ("depth 65536", fields(depth=65536), None, capi.RF_ERR_UNSUPPORTED, "depth * n_planes"),
    ("depth * planes 65536", fields(depth=4096, n_planes=16), None, capi.RF_ERR_UNSUPPORTED, "depth * n_planes"),
    ("depth * planes 65538", fields(depth=21846, n_planes=3), None, capi.RF_ERR_UNSUPPORTED, "depth * n_planes"),
    ("width 0", fields(width=0), None, capi.RF_ERR_INVALID_ARG, "positive"),
    ("height 0", fields(height=0), None, capi.RF_ERR_INVALID_ARG, "positive"),
    ("depth 0", fields(depth=0), None, capi.RF_ERR_INVALID_ARG, "positive"),
    ("depth -1", fields(depth=-1), None, capi.RF_ERR_INVALID_ARG, "positive"),
    ("dtype f64", fields(dtype=capi.RF_F64), None, capi.RF_ERR_UNSUPPORTED, "dtype"),
    ("dtype f16", fields(dtype=capi.RF_F16), None, capi.RF_ERR_UNSUPPORTED, "dtype"),
    ("dim 3", None, ((3, 1, 0),), capi.RF_ERR_INVALID_ARG, "dim"),
    ("dim -1", None, ((-1, 1, 0),), capi.RF_ERR_INVALID_ARG, "dim"),
    ("abi", fields(abi=capi.RF_ABI - 1), None, capi.RF_ERR_INVALID_ARG, "abi"),
    ("n_scans 0", fields(n_scans=0), None, capi.RF_ERR_INVALID_ARG, "n_scans"),
    ("n_scans 9", None, tuple((2, 1, 0) for _ in range(9)), capi.RF_ERR_INVALID_ARG, "n_scans"),
    ("n_planes 0", fields(n_planes=0), None, capi.RF_ERR_INVALID_ARG, "n_planes"),
    ("n_planes 17", fields(n_planes=capi.RF_MAX_PLANES + 1), None, capi.RF_ERR_INVALID_ARG, "n_planes"),
    ("n_weights 0", fields(n_weights=0), None, capi.RF_ERR_INVALID_ARG, "n_weights"),
    ("n_weights 9", fields(n_weights=capi.RF_VAR_MAX_SCANS + 1), None, capi.RF_ERR_INVALID_ARG, "n_weights"),
    ("weights 1 of 1", None, ((2, 1, 1),), capi.RF_ERR_INVALID_ARG, "weights"),
    ("flags", fields(flags=1), None, capi.RF_ERR_INVALID_ARG, "flags"),
    ("null scans", fields(scans=ctypes.POINTER(capi.VarScanDesc)()), None, capi.RF_ERR_INVALID_ARG, "scans"),
])
def test_refusals(what, edit, scans, status, text):
    got, message = raw_create(edit or (lambda d: None), scans or ((2, 1, 0),))
    assert got == status, f"{what}: status {got} ({message})"
    assert text in message, f"{what}: the message does not name the limit: {message!r}"


def test_null_arguments():
    h = ctypes.c_void_p()
    assert capi.lib().rf_var_plan_create_volume(None, ctypes.byref(h)) == capi.RF_ERR_INVALID_ARG
    assert capi.lib().rf_smooth_plan_create_volume(None, ctypes.byref(h)) == capi.RF_ERR_INVALID_ARG


def test_the_image_entry_point_still_refuses_three_dimensions():
    with pytest.raises(rfa.RecFilterError) as e:
        rfa.VarPlan((8, 40, 64), [PX], device=HOST)
    assert e.value.status == capi.RF_ERR_UNSUPPORTED


# ---- launches and workspace -----------------------------------------------------------------------------------------------------
def names_of(plan, backward=None):
    """the launch names of a host-only plan: the timed entry points fill names_out before they refuse to run"""
    n = plan.num_kernels if backward is None else plan.backward_num_kernels(backward)
    ms, names = (ctypes.c_float * n)(), (ctypes.c_char_p * n)()
    nulls = lambda k: (ctypes.c_void_p * k)()      # noqa: E731
    if backward is None:
        status = capi.lib().rf_var_plan_execute_timed(plan._h, nulls(plan.planes), nulls(plan.n_weights), nulls(plan.planes), None, ms, names, n)
    else:
        status = capi.lib().rf_var_plan_backward_timed(plan._h, nulls(plan.planes), nulls(plan.n_weights), nulls(plan.planes), nulls(plan.planes),
                                                       (ctypes.c_void_p * plan.n_weights)(*([1] * plan.n_weights)) if backward else None, None, ms, names, n)
    assert status == capi.RF_ERR_HIP
    return [v.decode() for v in names]


@pytest.mark.parametrize("name", list(SCAN_LISTS))
def test_num_kernels_and_names(name):
    scans = SCAN_LISTS[name]
    axis = "xyz"
    with host_plan((70, 66, 68), scans) as plan:
        assert plan.shape == (70, 66, 68)
        assert plan.num_kernels == 3 * STAGES[name]
        assert plan.backward_num_kernels(False) == 3 * len(scans)
        assert plan.backward_num_kernels(True) == 7 * len(scans)
        got = names_of(plan)
        assert got[1::3] == ["var_carry"] * STAGES[name]
        assert all(a.startswith("var_tails_") and b == "var_pass2_" + a[-1] for a, b in zip(got[0::3], got[2::3]))
        if STAGES[name] == len(scans):
            assert [a[-1] for a in got[0::3]] == [axis[d] for d, _, _ in scans]
        want = []
        for d, _, _ in reversed(scans):
            want += [f"var_adj_tails_{axis[d]}", "var_carry", f"var_adj_pass2_{axis[d]}"]
        assert names_of(plan, backward=False) == want
        with_grad = names_of(plan, backward=True)
        forward = [n for d, _, _ in scans for n in (f"var_tails_{axis[d]}", "var_carry", f"var_pass2_{axis[d]}")]
        assert with_grad[:len(forward)] == forward
        assert with_grad[len(forward) + 3::4] == [f"var_grad_{axis[d]}" for d, _, _ in reversed(scans)]


def test_the_full_list_is_three_pair_stages():
    with host_plan((70, 66, 68), SCAN_LISTS["+x-x+y-y+z-z"]) as plan:
        assert names_of(plan) == ["var_tails_x", "var_carry", "var_pass2_x", "var_tails_y", "var_carry", "var_pass2_y",
                                  "var_tails_z", "var_carry", "var_pass2_z"]


def slots_of(shape, scans):
    D, H, W = shape
    n = {0: W, 1: H, 2: D}
    return max(-(-n[d] // 64) * (W * H * D // n[d]) for d in {d for d, _, _ in scans})


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("name", ["+z-z", "+x-x", "+y", "+x-x+y-y+z-z"])
@pytest.mark.parametrize("shape", [(8, 40, 64), (70, 66, 68), (1024, 4, 8), (3, 130, 132), (1, 40, 64), (512, 512, 512), (64, 2048, 2048)])
def test_workspace_is_exact(shape, name, planes):
    scans = SCAN_LISTS[name]
    with host_plan(shape, scans, planes=planes) as plan:
        assert plan.workspace_bytes == 4 * planes * (5 + 2) * slots_of(shape, scans)
        assert plan.backward_workspace_bytes(True) == (len(scans) + 1) * planes * int(np.prod(shape)) * 4
        assert plan.backward_workspace_bytes(False) == 0


def test_host_only_plan_refuses_to_run():
    with host_plan((8, 40, 64), [PZ, MZ]) as plan:
        for call in (lambda: plan.execute([], [], []), lambda: plan.execute_timed([], [], []),
                     lambda: plan.execute_power([], [], [0.5, 0.5, 0.5], []), lambda: plan.backward(None, [], [], None, None),
                     lambda: plan.backward_power(None, [], [0.5, 0.5, 0.5], [], None, None)):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == capi.RF_ERR_HIP


def test_abi_revision_is_unchanged():
    assert capi.RF_ABI == 3
    assert b"abi 3" in capi.lib().rf_version()
    for name in ("rf_var_plan_create_volume", "rf_var_distances_volume", "rf_smooth_plan_create_volume"):
        assert name in capi.EXPORTED_SYMBOLS


# ---- the smoothing plan ---------------------------------------------------------------------------------------------------------
def smooth_host(shape, **kw):
    return rfa.SmoothPlan.volume(shape, device=HOST, **kw)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("u8", [False, True])
def test_smoothing_plan_launches_and_workspace(K, u8):
    import torch
    shape, planes = (20, 66, 68), 3
    with smooth_host(shape, planes=planes, iterations=K, image_dtype=torch.uint8 if u8 else torch.float32) as plan:
        assert plan.num_kernels == 1 + 9 * K
        assert len(plan.bases) == K
        samples = int(np.prod(shape))
        inner = 4 * planes * 7 * slots_of(shape, SCAN_LISTS["+x-x+y-y+z-z"])
        assert plan.workspace_bytes == 4 * samples * (3 + (planes if u8 else 0)) + inner
        assert plan.backward_num_kernels(False) == 0 and plan.backward_num_kernels(True) == 0
        assert plan.backward_workspace_bytes(True) == 0
        n = plan.num_kernels
        ms, names = (ctypes.c_float * n)(), (ctypes.c_char_p * n)()
        nulls = (ctypes.c_void_p * planes)()
        assert capi.lib().rf_smooth_plan_execute_timed(plan._h, nulls, None, nulls, None, ms, names, n) == capi.RF_ERR_HIP
        per_iteration = ["var_tails_x", "var_carry", "var_pass2_x", "var_tails_y", "var_carry", "var_pass2_y", "var_tails_z", "var_carry", "var_pass2_z"]
        assert [v.decode() for v in names] == ["var_distances_volume"] + per_iteration * K


def test_smoothing_plan_backward_is_unsupported():
    with smooth_host((8, 40, 64)) as plan:
        for edges in (False, True):
            with pytest.raises(rfa.RecFilterError) as e:
                plan.backward(None, None, None, None, None, edges=edges)
            assert e.value.status == capi.RF_ERR_UNSUPPORTED
        n = 4
        ms, names = (ctypes.c_float * n)(), (ctypes.c_char_p * n)()
        nulls = (ctypes.c_void_p * 1)()
        assert capi.lib().rf_smooth_plan_backward_timed(plan._h, nulls, None, nulls, nulls, None, 0, None, ms, names, n) == capi.RF_ERR_UNSUPPORTED


@pytest.mark.parametrize("what,shape,kw,status,text", [
    ("spacing 0", (8, 40, 64), dict(spacing_z=0.0), capi.RF_ERR_INVALID_ARG, "spacing_z"),
    ("spacing -1", (8, 40, 64), dict(spacing_z=-1.0), capi.RF_ERR_INVALID_ARG, "spacing_z"),
    ("spacing inf", (8, 40, 64), dict(spacing_z=float("inf")), capi.RF_ERR_INVALID_ARG, "spacing_z"),
    ("spacing nan", (8, 40, 64), dict(spacing_z=float("nan")), capi.RF_ERR_INVALID_ARG, "spacing_z"),
    ("width 66", (8, 40, 66), {}, capi.RF_ERR_UNSUPPORTED, "multiple of 4"),
    ("depth 0", (0, 40, 64), {}, capi.RF_ERR_INVALID_ARG, "positive"),
    ("depth * planes", (21846, 8, 8), dict(planes=3), capi.RF_ERR_UNSUPPORTED, "depth * n_planes"),
    ("width * height", (1, (1 << 15) + 1, 1 << 15), {}, capi.RF_ERR_UNSUPPORTED, "width * height"),
    ("iterations 0", (8, 40, 64), dict(iterations=0), capi.RF_ERR_INVALID_ARG, "iterations"),
    ("sigma_r 0", (8, 40, 64), dict(sigma_r=0.0), capi.RF_ERR_INVALID_ARG, "sigma_r"),
])
def test_smoothing_plan_refusals(what, shape, kw, status, text):
    with pytest.raises(rfa.RecFilterError) as e:
        smooth_host(shape, **kw)
    assert e.value.status == status, f"{what}: {e.value}"
    assert text in str(e.value), f"{what}: {e.value}"


@pytest.mark.parametrize("shape,planes", [((512, 512, 512), 1), ((64, 2048, 2048), 1), ((21845, 8, 8), 3)])
def test_smoothing_plan_accepts_the_large_volumes(shape, planes):
    with smooth_host(shape, planes=planes, spacing_z=2.5) as plan:
        assert plan.num_kernels == 28


# ---- rf_var_distances_volume: what is decided before any HIP call ------------------------------------------------------------------
def raw_distances(n_guide=1, u8=0, W=64, H=40, D=8, scale=1.0, spacing=1.0, guide=0x1000, dx=0x100000, dy=0x200000, dz=0x300000):
    """the status and message of a call that must be refused: the addresses are never dereferenced"""
    guides = (ctypes.c_void_p * max(n_guide, 1))(*([guide] * max(n_guide, 1)))
    status = capi.lib().rf_var_distances_volume(guides, n_guide, u8, W, H, D, scale, spacing, dx, dy, dz, -1, None)
    return status, capi.lib().rf_last_error_string().decode()


@pytest.mark.parametrize("what,kw,status,text", [
    ("n_guide 0", dict(n_guide=0), capi.RF_ERR_INVALID_ARG, "n_guide"),
    ("n_guide 17", dict(n_guide=17), capi.RF_ERR_INVALID_ARG, "n_guide"),
    ("depth 0", dict(D=0), capi.RF_ERR_INVALID_ARG, "positive"),
    ("null dz", dict(dz=None), capi.RF_ERR_INVALID_ARG, "null"),
    ("null guide", dict(guide=None), capi.RF_ERR_INVALID_ARG, "null"),
    ("scale -1", dict(scale=-1.0), capi.RF_ERR_INVALID_ARG, "scale"),
    ("scale nan", dict(scale=float("nan")), capi.RF_ERR_INVALID_ARG, "scale"),
    ("spacing 0", dict(spacing=0.0), capi.RF_ERR_INVALID_ARG, "spacing_z"),
    ("spacing -2", dict(spacing=-2.0), capi.RF_ERR_INVALID_ARG, "spacing_z"),
    ("spacing inf", dict(spacing=float("inf")), capi.RF_ERR_INVALID_ARG, "spacing_z"),
    ("width 66", dict(W=66), capi.RF_ERR_UNSUPPORTED, "multiple of 4"),
    ("depth 65536", dict(D=65536), capi.RF_ERR_UNSUPPORTED, "depth"),
    ("width * height", dict(W=1 << 15, H=(1 << 15) + 1, D=1), capi.RF_ERR_UNSUPPORTED, "width * height"),
    ("misaligned dz", dict(dz=0x300004), capi.RF_ERR_INVALID_ARG, "aligned"),
    ("misaligned f32 guide", dict(guide=0x1004), capi.RF_ERR_INVALID_ARG, "aligned"),
    ("misaligned u8 guide", dict(guide=0x1002, u8=1), capi.RF_ERR_INVALID_ARG, "aligned"),
    ("dz is dx", dict(dz=0x100000), capi.RF_ERR_INVALID_ARG, "overlap"),
    ("guide inside dy", dict(guide=0x200100), capi.RF_ERR_INVALID_ARG, "overlap"),
])
def test_distance_refusals(what, kw, status, text):
    got, message = raw_distances(**kw)
    assert got == status, f"{what}: status {got} ({message})"
    assert text in message, f"{what}: {message!r}"


# ---- the loops ------------------------------------------------------------------------------------------------------------------
def test_loops_move_the_axis():
    """a scan along an axis of a volume is the 2-D loops' scan of every line along that axis"""
    import var_grad_loops as loops
    rng = np.random.default_rng(5)
    x, w = rng.random((5, 6, 8)), rng.random((5, 6, 8))
    for dim, axis in ((0, 2), (1, 1), (2, 0)):
        for causal in (True, False):
            got = vloops.reference([x], [w], [(dim, causal, 0)], np.float64)[0]
            for i in range(3):
                for j in range(4):
                    index = [i, j]
                    index.insert(axis, slice(None))
                    line, wl = x[tuple(index)][None, :], w[tuple(index)][None, :]
                    want = loops.scan(line, loops.masked_weights(wl, np.float64), causal)[0]
                    np.testing.assert_array_equal(got[tuple(index)], want)


@pytest.mark.parametrize("name", ["+z-z", "-z+z", "+x-x+y-y+z-z", "+z-z two weights"])
def test_gradient_loops_against_central_differences(name):
    """tests/var_volume_loops.py on a (5, 6, 8) volume in f64: the directional derivative of L = sum(g * out) along random
    directions in the volume, in the weights and in the exponents"""
    shape, scans, h = (5, 6, 8), SCAN_LISTS[name], 1e-6
    rng = np.random.default_rng(568)
    x, g, dx = (rng.random(shape) * 2 - 1 for _ in range(3))
    ws = [rng.random(shape) * 0.9 + 0.05 for _ in range(3)]
    ds = [1 + 3 * rng.random(shape) for _ in range(3)]
    dws = [rng.random(shape) * 2 - 1 for _ in range(3)]
    bases = [0.8, 0.97, 0.9]

    def loss(xx, weights):
        return float(np.sum(g * vloops.reference([xx], weights, scans, np.float64)[0]))

    def shifted(volumes, t):
        return [p + t * d for p, d in zip(volumes, dws)]

    def inner(grads):
        """sum over the weight volumes of <gradient, direction>, element 0 along the scanned axis left out (it is never read)"""
        total = 0.0
        for k in sorted({k for _, _, k in scans}):
            dims = {d for d, _, kk in scans if kk == k}
            assert len(dims) == 1
            axis = vloops.AXIS[dims.pop()]
            first = np.take(grads[k], 0, axis=axis)
            assert np.all(first == 0)
            total += float(np.sum(np.delete(grads[k] * dws[k], 0, axis=axis)))
        return total
    gin, gw = vloops.backward([x], ws, scans, [g], np.float64)
    assert abs((loss(x + h * dx, ws) - loss(x - h * dx, ws)) / (2 * h) - float(np.sum(gin[0] * dx))) < 1e-7
    assert abs((loss(x, shifted(ws, h)) - loss(x, shifted(ws, -h))) / (2 * h) - inner(gw)) < 1e-7

    def power(volumes):
        return [np.exp2(d * np.log2(np.float64(np.float32(b)))) for d, b in zip(volumes, bases)]
    _, gd = vloops.power_backward([x], ds, bases, scans, [g], np.float64)
    assert abs((loss(x, power(shifted(ds, h))) - loss(x, power(shifted(ds, -h)))) / (2 * h) - inner(gd)) < 1e-7


def test_distance_loops():
    rng = np.random.default_rng(9)
    g = rng.random((2, 3, 4, 8))
    dx, dy, dz = vloops.distances(g, 0.5, 2.5, np.float64)
    assert np.all(dx[:, :, 0] == 1) and np.all(dy[:, 0, :] == 1) and np.all(dz[0] == 2.5)
    assert dz[2, 1, 3] == 2.5 + 0.5 * (abs(g[0, 2, 1, 3] - g[0, 1, 1, 3]) + abs(g[1, 2, 1, 3] - g[1, 1, 1, 3]))
    assert dx[2, 1, 3] == 1 + 0.5 * (abs(g[0, 2, 1, 3] - g[0, 2, 1, 2]) + abs(g[1, 2, 1, 3] - g[1, 2, 1, 2]))
    assert dy[2, 1, 3] == 1 + 0.5 * (abs(g[0, 2, 1, 3] - g[0, 2, 0, 3]) + abs(g[1, 2, 1, 3] - g[1, 2, 0, 3]))
