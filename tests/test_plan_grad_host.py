"""rf_plan_backward without a GPU: the mathematics (tests/plan_grad_loops.py against central differences of the CPU oracle and
the adjoint identity), the refusals of the C ABI on host-only plans, and the Python argument checks."""
import ctypes

import numpy as np
import pytest

import oracle
import plan_grad_loops as pgl
import ref_cases as rc
import recfilter_amd as rfa
from recfilter_amd import capi

X, Y, Z, C, A = rc.X, rc.Y, rc.Z, rc.C, rc.A

CASES = {
    "signal_40": dict(shape=(40,), scans=[(X, C, [0.5, 0.4, -0.1]), (X, A, [0.6, 0.3]), (X, C, rc.GAUSS3)]),
    "image_7x9_gauss2": dict(shape=(7, 9), scans=rc.xy_pm(rc.GAUSS2)),
    "image_7x9_gauss3": dict(shape=(7, 9), scans=rc.xy_pm(rc.GAUSS3)),
    "volume_5x6x8": dict(shape=(5, 6, 8), scans=[(X, C, [0.5, 0.4, -0.1]), (X, A, rc.GAUSS3), (Y, A, [0.6, 0.3]), (Y, C, rc.GAUSS2),
                                                 (Z, C, rc.GAUSS3), (Z, A, [0.9, 0.05])]),
    "image_7x9_pointwise": dict(shape=(7, 9), scans=rc.xy_pm(rc.GAUSS2), prologue=(0.5, 0.25), epilogue=(-0.7, 1.7, 0.1)),
}


def _data(shape):
    x = np.random.default_rng(11).random(shape)
    g = np.random.default_rng(12).random(shape) - 0.5
    return x, g


def _loss(x, g, scans, clamped, prologue, epilogue):
    return float(np.sum(g * pgl.forward(x, scans, clamped, prologue, epilogue)))


@pytest.mark.parametrize("clamped", [False, True], ids=["zero", "clamped"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_coefficient_gradients_match_central_differences(name, clamped):
    """every coefficient of every scan: the deviation from a central difference of the oracle is O(h^2) -- it falls about
    256-fold when the (representable) step goes from 2^-10 to 2^-14 -- or sits at the rounding floor of the difference"""
    case = CASES[name]
    scans, pro, epi = case["scans"], case.get("prologue"), case.get("epilogue")
    x, g = _data(case["shape"])
    _, rows, mags = pgl.backward(x, scans, clamped, g, np.float64, pro, epi)
    for s, (dim, causal, coeff) in enumerate(scans):
        for j in range(len(coeff)):
            dev = []
            for h in (2.0 ** -10, 2.0 ** -14):
                def shifted(delta):
                    c = [float(np.float32(v)) for v in coeff]
                    c[j] += delta
                    assert float(np.float32(c[j])) == c[j], "the step must be representable"
                    return scans[:s] + [(dim, causal, c)] + scans[s + 1:]
                fd = (_loss(x, g, shifted(h), clamped, pro, epi) - _loss(x, g, shifted(-h), clamped, pro, epi)) / (2 * h)
                dev.append(abs(fd - rows[s, j]) / mags[s, j])
            # (the truncation term h^2 f'''/6 of a third-order Gaussian on 40 samples reaches 3e-4 at h = 2^-10, 1.3e-6 at 2^-14)
            assert dev[0] < 1e-2 and dev[1] < 1e-5, (name, s, j, dev)
            assert dev[1] < dev[0] / 100 or dev[1] < 1e-9, (name, s, j, dev)
        assert not rows[s, len(coeff):].any()


@pytest.mark.parametrize("clamped", [False, True], ids=["zero", "clamped"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_adjoint_identity(name, clamped):
    """<F(x), g> = <x, F^T(g)> for the linear part of the filter, to 1e-12"""
    case = CASES[name]
    scans, pro, epi = case["scans"], case.get("prologue"), case.get("epilogue")
    if pro is not None:
        pro, epi = (pro[0], 0.0), (epi[0], epi[1], 0.0)        # the biases are not part of the linear map
    x, g = _data(case["shape"])
    gin, _, _ = pgl.backward(x, scans, clamped, g, np.float64, pro, epi)
    lhs, rhs = float(np.sum(pgl.forward(x, scans, clamped, pro, epi) * g)), float(np.sum(x * gin))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)


def test_input_gradient_matches_central_differences():
    x, g = _data((7, 9))
    scans = rc.xy_pm(rc.GAUSS3)
    for clamped in (False, True):
        gin, _, _ = pgl.backward(x, scans, clamped, g)
        for idx in [(0, 0), (3, 4), (6, 8), (0, 5)]:
            e = np.zeros_like(x)
            e[idx] = 2.0 ** -10
            fd = (_loss(x + e, g, scans, clamped, None, None) - _loss(x - e, g, scans, clamped, None, None)) / 2.0 ** -9
            assert abs(fd - gin[idx]) < 1e-11, (clamped, idx)


def test_f32_loops_stay_near_the_truth():
    x, g = _data((7, 9))
    for clamped in (False, True):
        g64, r64, m64 = pgl.backward(x.astype(np.float32), rc.xy_pm(rc.GAUSS2), clamped, g.astype(np.float32), np.float64)
        g32, r32, _ = pgl.backward(x.astype(np.float32), rc.xy_pm(rc.GAUSS2), clamped, g.astype(np.float32), np.float32)
        assert g32.dtype == np.float32
        assert np.max(np.abs(g32 - g64)) < 1e-5
        assert np.max(np.abs(r32 - r64)[:, :3] / m64[:, :3]) < 1e-5


# ---- the refusals of the C ABI, on host-only plans --------------------------------------------------------------------------
GAUSS2_XY = rc.xy_pm(rc.GAUSS2)
BASE = 0x7f0000000000           # addresses that are never dereferenced: every refusal is decided before any HIP call


def _planes(n, shape, offset=0, itemsize=4):
    step = (int(np.prod(shape)) * itemsize + 255) // 256 * 256
    return (ctypes.c_void_p * n)(*[BASE + offset + i * step for i in range(n)])


def _host_plan(shape=(64, 256), scans=GAUSS2_XY, **kw):
    return rfa.Plan(shape, scans, device=capi.RF_DEVICE_HOST_ONLY, **kw)


def _call(plan, pin, pgo, pgi, coeffs=None):
    rc_ = capi.lib().rf_plan_backward(plan._h, pin, pgo, pgi, ctypes.c_void_p(coeffs) if coeffs else None, None)
    return rc_, capi.lib().rf_last_error_string().decode()


FAR = 1 << 32


def _refusal(plan, want, pin=None, pgo="default", pgi="default", coeffs=None, shape=(64, 256)):
    n = plan.planes
    pgo = _planes(n, shape, 0) if pgo == "default" else pgo
    pgi = _planes(n, shape, FAR) if pgi == "default" else pgi
    state = (plan.workspace_bytes, plan.num_kernels, plan.debug_buffers())
    status, message = _call(plan, pin, pgo, pgi, coeffs)
    assert status == want, (status, message)
    assert message
    assert state == (plan.workspace_bytes, plan.num_kernels, plan.debug_buffers())
    return message


def test_refusals_in_order():
    shape = (64, 256)
    inp, coeffs = _planes(1, shape, 2 * FAR), BASE + 3 * FAR
    with _host_plan() as plan:
        # null arguments and in_planes that does not match grad_coeffs
        _refusal(plan, capi.RF_ERR_INVALID_ARG, pgo=None)
        _refusal(plan, capi.RF_ERR_INVALID_ARG, pgi=None)
        _refusal(plan, capi.RF_ERR_INVALID_ARG, pgi=(ctypes.c_void_p * 1)(None))
        _refusal(plan, capi.RF_ERR_INVALID_ARG, coeffs=coeffs)                    # coefficients without inputs
        _refusal(plan, capi.RF_ERR_INVALID_ARG, pin=inp)                          # inputs without coefficients
        # misaligned planes on the fused path
        assert plan.path == capi.RF_PATH_TILED_FUSED
        assert "aligned" in _refusal(plan, capi.RF_ERR_INVALID_ARG, pgi=_planes(1, shape, FAR + 4))
        assert "aligned" in _refusal(plan, capi.RF_ERR_INVALID_ARG, pin=_planes(1, shape, 2 * FAR + 8), coeffs=coeffs)
        # a written plane that overlaps another plane of the call
        assert "overlaps" in _refusal(plan, capi.RF_ERR_INVALID_ARG, pgi=_planes(1, shape, 64))
        assert "overlaps" in _refusal(plan, capi.RF_ERR_INVALID_ARG, pin=_planes(1, shape, FAR + 1024), coeffs=coeffs)
        assert "overlaps" in _refusal(plan, capi.RF_ERR_INVALID_ARG, pin=inp, coeffs=BASE + FAR + 16)
        # in place is allowed: the next refusal in line is the host-only one
        same = _planes(1, shape, 0)
        _refusal(plan, capi.RF_ERR_HIP, pgo=same, pgi=same)
        _refusal(plan, capi.RF_ERR_HIP)
        _refusal(plan, capi.RF_ERR_HIP, pin=inp, coeffs=coeffs)
    with _host_plan(planes=2) as plan:
        both = _planes(2, shape, FAR)
        both[1] = both[0]
        assert "overlaps" in _refusal(plan, capi.RF_ERR_INVALID_ARG, pgi=both)


@pytest.mark.parametrize("n", [1, 2], ids=["one_plane", "two_planes"])
def test_aliasing_rule_names_both_planes(n):
    """a written plane (grad_in, grad_coeffs) is disjoint from every other plane of the call, except that grad_in[p] may be
    exactly grad_out[p]: every refusal names both arrays and both plane indices"""
    shape = (64, 64)
    plane_bytes, coeff_bytes = 64 * 64 * 4, len(GAUSS2_XY) * (1 + capi.RF_MAX_ORDER) * 8
    gout, gin, inp = (lambda: _planes(n, shape, 0)), (lambda: _planes(n, shape, FAR)), (lambda: _planes(n, shape, 2 * FAR))
    coeffs = BASE + 3 * FAR
    last = n - 1

    def moved(planes, index, address):
        planes[index] = address
        return planes

    def refused(a, i, b, j, **call):
        message = _refusal(plan, capi.RF_ERR_INVALID_ARG, shape=shape, **call)
        one, other = f"{a} plane {i}", f"{b} plane {j}"
        assert message.startswith(f"{one} overlaps {other}") or message.startswith(f"{other} overlaps {one}"), message

    with _host_plan(shape=shape, planes=n) as plan:
        # grad_in against grad_out: its own plane unless exactly, another plane even exactly
        refused("grad_in", last, "grad_out", last, pgi=moved(gin(), last, gout()[last] + 64))
        refused("grad_in", 0, "grad_out", 0, pgi=moved(gin(), 0, gout()[0] - plane_bytes + 16))
        if n == 2:
            refused("grad_in", 0, "grad_out", 1, pgi=moved(gin(), 0, gout()[1]))
            refused("grad_in", 1, "grad_out", 0, pgi=moved(gin(), 1, gout()[0] - plane_bytes + 16))
            # grad_in against grad_in
            refused("grad_in", 0, "grad_in", 1, pgi=moved(gin(), 1, gin()[0]))
            refused("grad_in", 0, "grad_in", 1, pgi=moved(gin(), 1, gin()[0] + 1024))
        # grad_in against in (read only with the coefficients)
        refused("grad_in", last, "in", 0, pin=inp(), coeffs=coeffs, pgi=moved(gin(), last, inp()[0] - 256))
        refused("grad_in", 0, "in", last, pin=inp(), coeffs=coeffs, pgi=moved(gin(), 0, inp()[last]))
        # grad_coeffs, n_scans rows of 1 + RF_MAX_ORDER doubles, against each of the three: its first and its last byte
        for array, noun in ((gout(), "grad_out"), (gin(), "grad_in"), (inp(), "in")):
            refused("grad_coeffs", 0, noun, last, pin=inp(), coeffs=array[last] + plane_bytes - 8)
            refused("grad_coeffs", 0, noun, 0, pin=inp(), coeffs=array[0] - coeff_bytes + 8)
            _refusal(plan, capi.RF_ERR_HIP, shape=shape, pin=inp(), coeffs=array[0] - coeff_bytes)
            _refusal(plan, capi.RF_ERR_HIP, shape=shape, pin=inp(), coeffs=array[last] + plane_bytes)
        # in place, plane for plane and exactly, is accepted as far as the host-only refusal
        _refusal(plan, capi.RF_ERR_HIP, shape=shape, pgo=gout(), pgi=gout())
        _refusal(plan, capi.RF_ERR_HIP, shape=shape, pgo=gout(), pgi=gout(), pin=inp(), coeffs=coeffs)
        _refusal(plan, capi.RF_ERR_HIP, shape=shape, pgo=gout(), pgi=moved(gin(), last, gout()[last]))


def test_refusals_of_the_description():
    shape = (64, 256)
    inp, coeffs = _planes(1, shape, 2 * FAR), BASE + 3 * FAR
    with _host_plan(dtype=np.float64) as plan:
        assert "f32" in _refusal(plan, capi.RF_ERR_UNSUPPORTED, pgo=_planes(1, shape, 0, 8), pgi=_planes(1, shape, FAR, 8))
        assert plan.backward_num_kernels(False) == 0
    with _host_plan(dtype=np.float16) as plan:
        _refusal(plan, capi.RF_ERR_UNSUPPORTED)
    with _host_plan(input_dtype=np.uint8) as plan:
        assert "byte" in _refusal(plan, capi.RF_ERR_UNSUPPORTED)
    with _host_plan(flags=capi.RF_PLAN_FORCE_EXCHANGE) as plan:
        assert "sharded" in _refusal(plan, capi.RF_ERR_UNSUPPORTED)
    with _host_plan(shard_world=2, shard_rank=0) as plan:
        assert "sharded" in _refusal(plan, capi.RF_ERR_UNSUPPORTED)
    with _host_plan(prologue=(0.5, 0.1)) as plan:
        assert "pointwise" in _refusal(plan, capi.RF_ERR_UNSUPPORTED, pin=inp, coeffs=coeffs)
        _refusal(plan, capi.RF_ERR_HIP)                                          # without coefficients the stages compose
    with _host_plan(epilogue=(-0.7, 1.7, 0.1)) as plan:
        same = _planes(1, shape, 0)
        assert "epilogue" in _refusal(plan, capi.RF_ERR_INVALID_ARG, pgo=same, pgi=same)
    with _host_plan(shape=(3, 256), scans=rc.xy_pm(rc.GAUSS3), clamped=True) as plan:      # 3 rows, order 3 along y
        assert "clamped" in _refusal(plan, capi.RF_ERR_UNSUPPORTED, shape=(3, 256))
    with _host_plan(scans=[(X, C, [0.0, 0.5])], clamped=True) as plan:
        assert "feed-forward" in _refusal(plan, capi.RF_ERR_UNSUPPORTED)
    with _host_plan(scans=[(X, C, [0.0, 0.5])], clamped=False) as plan:          # a zero border does not mind
        _refusal(plan, capi.RF_ERR_HIP)
    with _host_plan(clamped=True, prologue=(0.5, 0.0)) as plan:
        assert "pointwise" in _refusal(plan, capi.RF_ERR_UNSUPPORTED)


def test_host_only_queries():
    """a host-only plan answers the backward's queries (its child plans are host-only too) and keeps the forward's"""
    with _host_plan() as plan, _host_plan(clamped=True) as clamped:
        for p in (plan, clamped):
            before = (p.workspace_bytes, p.num_kernels, p.debug_buffers(), p.table("scans").tolist())
            n1, n3 = p.backward_num_kernels(False), p.backward_num_kernels(True)
            assert n1 > 0 and n3 > n1
            assert p.backward_workspace_bytes(False) == 0
            assert p.backward_workspace_bytes(True) == (4 + 1) * 64 * 256 * 4 + 1024 * 33 * 8
            assert before == (p.workspace_bytes, p.num_kernels, p.debug_buffers(), p.table("scans").tolist())
        # route 1 is ONE plan of the transposed scans: as many launches as the forward of that list
        transposed = [(d, not c, w) for d, c, w in reversed(GAUSS2_XY)]
        with _host_plan(scans=transposed) as t:
            assert plan.backward_num_kernels(False) == t.num_kernels
        # route 2: per scan a child plan and the border launch; route 3 adds the forward and two launches per scan
        assert clamped.backward_num_kernels(True) - plan.backward_num_kernels(True) >= 4
    assert capi.lib().rf_plan_backward_num_kernels(None, 0) == 0
    assert capi.lib().rf_plan_backward_workspace_bytes(None, 1) == 0


def test_python_argument_checks():
    import torch
    with _host_plan() as plan:
        g = torch.zeros(64, 256)
        with pytest.raises(ValueError, match="inputs"):
            plan.backward([g], coeff_grads=True)
        with pytest.raises(ValueError, match="coeff_grads"):
            plan.backward([g], inputs=[g])
        with pytest.raises(ValueError, match="device tensors"):
            plan.backward([g])
        with pytest.raises(ValueError, match="planes"):
            plan.backward([g, g])
        with pytest.raises(ValueError, match="shape"):
            plan.backward([torch.zeros(64, 128)])
        with pytest.raises(ValueError, match="planes"):
            plan.apply([g, g])
    with pytest.raises(ValueError, match="coefficient tensors"):
        rfa.recursive_filter(torch.zeros(4, 4), [(0, True)], [])
    with pytest.raises(TypeError, match="f32 device tensor"):
        rfa.recursive_filter(torch.zeros(4, 4), [(0, True)], [torch.tensor([1.0, 0.5])])
