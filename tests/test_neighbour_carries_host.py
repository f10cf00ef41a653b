"""Neighbour-form carries of the fused x/y path (plan_fused.cpp, neighbour_carry_bound), checked without a GPU.

For a filter that decays within a tile, the carry scans along a dimension add nothing an f32 result can see beyond the
nearest tile: the plan then completes the carries of a dimension with one scan, or with a causal scan followed by an
anticausal one, from the neighbouring tiles' tails alone (no carry_x / carry_y launch).  Here:
  * the decision and the bound rf_plan_table("neighbour_carries") reports, on host-only plans, against the same bound
    computed in numpy -- from the plan's own tables and, for the transitions across a tile, from the coefficients alone;
  * the algebra: the emulator of the fused path (tests/fused_emulator.py) with the transfers the neighbour form drops
    taken out (A^L = 0 in the carry stages) against the full emulator and against the f64 oracle."""
import numpy as np
import pytest

import oracle
import ref_cases as rc
import recfilter_amd as rfa
from recfilter_amd import capi
from fused_emulator import FusedEmu

HOST = dict(device=capi.RF_DEVICE_HOST_ONLY)
BOUND = 2.0 ** -32
FUSED = capi.RF_PATH_TILED_FUSED


def _nb(plan):
    bx, tx, by, ty = plan.table("neighbour_carries")
    return bx, bool(tx), by, bool(ty)


def _inf(m):
    return float(np.max(np.sum(np.abs(m), axis=-1)))


def _scan_matrices(coeff, T, clamped):
    """A (causal), A (anticausal) and W_v[0->1] (v = 0 interior tile, 2 last tile) of a causal + anticausal pair with the same
    coefficients over whole tiles of T samples, from the recurrences alone (not from the plan): the carry of a scan is its tail,
    the last k outputs in its direction, newest first; the anticausal scan of the last tile enters at a clamped border the way
    the oracle's loops do (taps beyond the border read the scan's first output; that first output reads the input there)."""
    c = np.asarray(coeff, dtype=np.float32).astype(np.float64)
    b, a = c[0], c[1:]
    k = len(a)

    def causal(x, carry):                      # y[n] = b x[n] + sum a_j y[n-1-j], y[-1-j] = carry[j]
        y = np.zeros(T)
        for n in range(T):
            y[n] = b * x[n] + sum(a[j] * (y[n - 1 - j] if n - 1 - j >= 0 else carry[j - n]) for j in range(k))
        return y

    def anticausal(x, carry, clamp):           # z[n] = b x[n] + sum a_j z[n+1+j], z[T+j] = carry[j] (or the clamped border)
        z = np.zeros(T)
        for n in range(T - 1, -1, -1):
            acc = b * x[n]
            for j in range(k):
                t = n + 1 + j
                if t < T:
                    acc += a[j] * z[t]
                elif clamp:
                    acc += a[j] * (x[T - 1] if n == T - 1 else z[T - 1])
                else:
                    acc += a[j] * carry[t - T]
            z[n] = acc
        return z

    E, zero = np.eye(k), np.zeros(T)
    A0 = np.stack([causal(zero, E[o])[::-1][:k] for o in range(k)], axis=1)                # tail r = y[T-1-r]
    A1 = np.stack([anticausal(zero, E[o], False)[:k] for o in range(k)], axis=1)           # tail r = z[r]
    W = {v: np.stack([anticausal(causal(zero, E[o]), np.zeros(k), clamped and v == 2)[:k] for o in range(k)], axis=1)
         for v in (0, 2)}
    return A0, A1, W


def _numpy_bound(coeff, T, clamped):
    """The neighbour form's bound, max(|A_0^L|, max_v |W_v[0->1] A_0^L| + |A_1^L|), computed independently of the plan."""
    A0, A1, W = _scan_matrices(coeff, T, clamped)
    return max(_inf(A0), max(_inf(W[v] @ A0) for v in (0, 2)) + _inf(A1))


def test_cfg3_takes_both_dimensions_and_the_bound_is_what_numpy_computes():
    c = rc.BASELINE_CONFIGS["cfg3_gaussian2_xy"]
    with rfa.Plan(c["shape"], c["scans"], clamped=c["clamped"], path=FUSED, **HOST) as plan:
        assert plan.tiles[:2] == (256, 128)
        bx, tx, by, ty = _nb(plan)
        assert tx and ty
        assert 0 <= bx <= BOUND and 0 <= by <= BOUND
        np.testing.assert_allclose(bx, _numpy_bound(rc.GAUSS2, 256, True), rtol=1e-6, atol=0)
        np.testing.assert_allclose(by, _numpy_bound(rc.GAUSS2, 128, True), rtol=1e-6, atol=0)
        # the plan's own tables are the same matrices as the recurrences (same tail convention)
        for dim, T in (("x", 256), ("y", 128)):
            A0, A1, W = _scan_matrices(rc.GAUSS2, T, True)
            np.testing.assert_allclose(plan.table("A_" + dim).reshape(2, 2, 2), np.stack([A0, A1]), rtol=1e-6, atol=1e-30)
            Wp = plan.table("W_" + dim).reshape(4, 2, 2, 2, 2)
            for v in (0, 2):
                np.testing.assert_allclose(Wp[v, 0, 1], W[v], rtol=1e-6, atol=1e-12)
    with rfa.Plan(c["shape"], c["scans"], clamped=c["clamped"], path=FUSED, flags=capi.RF_PLAN_FULL_CARRY_SCAN, **HOST) as plan:
        bx2, tx2, by2, ty2 = _nb(plan)
        assert not tx2 and not ty2 and bx2 == bx and by2 == by      # the flag keeps the scans; the bound is reported anyway


def test_cfg2_running_sums_take_neither():
    c = rc.BASELINE_CONFIGS["cfg2_summed_table"]
    with rfa.Plan(c["shape"], c["scans"], clamped=c["clamped"], path=FUSED, **HOST) as plan:
        bx, tx, by, ty = _nb(plan)
        assert not tx and not ty
        assert bx == pytest.approx(1.0) and by == pytest.approx(1.0)
    with rfa.Plan(c["shape"], c["scans"], clamped=c["clamped"], path=FUSED, dtype=np.int32, **HOST) as plan:
        assert _nb(plan) == (-1.0, False, -1.0, False)           # integer pixels: not even a bound


def test_gauss2_on_64_row_tiles_takes_x_only():
    with rfa.Plan((4096, 4096), rc.xy_pm(rc.GAUSS2), clamped=True, path=FUSED, flags=capi.RF_PLAN_TILE_ROWS(64), **HOST) as plan:
        assert plan.tiles[1] == 64
        bx, tx, by, ty = _nb(plan)
        assert tx and not ty
        assert by > BOUND
        np.testing.assert_allclose(by, _numpy_bound(rc.GAUSS2, 64, True), rtol=1e-6, atol=0)
        np.testing.assert_allclose(bx, _numpy_bound(rc.GAUSS2, 256, True), rtol=1e-6, atol=0)
    # GAUSS2 and GAUSS3 on 32-row tiles (what a small batched image takes) keep their y scans too
    for co in (rc.GAUSS2, rc.GAUSS3):
        with rfa.Plan((128, 512), rc.xy_pm(co), clamped=True, planes=3, path=FUSED, flags=capi.RF_PLAN_TILE_ROWS(32), **HOST) as plan:
            assert plan.tiles[1] == 32
            _, tx, _, ty = _nb(plan)
            assert tx and not ty


@pytest.mark.parametrize("scans,expect", [
    ([(0, True, [0.03, 0.97]), (1, True, [0.03, 0.97])], (False, False)),                      # a pole at 0.97 decays too slowly
    ([(0, True, [0.5, 0.5]), (0, True, [0.5, 0.5]), (1, False, [0.5, 0.5])], (False, True)),    # two causal x scans
    ([(0, False, rc.GAUSS2), (0, True, rc.GAUSS2), (1, True, rc.GAUSS2)], (False, True)),       # anticausal first
    (rc.xy_pm(rc.BICUBIC_COEFF), (True, True)),
    (rc.xy_pm(rc.GAUSS3), (True, True)),
], ids=["pole_097", "two_causal", "anticausal_first", "bicubic", "gauss3"])
def test_decision_per_dimension(scans, expect):
    with rfa.Plan((2048, 2048), scans, clamped=True, path=FUSED, flags=capi.RF_PLAN_TILE_ROWS(128), **HOST) as plan:
        assert plan.tiles[1] == 128
        bx, tx, by, ty = _nb(plan)
        assert (tx, ty) == expect, (bx, by)


def test_sharded_and_volume_plans_keep_their_scans():
    g = rc.xy_pm(rc.GAUSS2)
    with rfa.Plan((1024, 2048), g, clamped=True, path=FUSED, shard_rank=0, shard_world=2, **HOST) as plan:
        assert _nb(plan) == (-1.0, False, -1.0, False)
    with rfa.Plan((64, 1024, 1024), g + [(2, True, rc.GAUSS2)], clamped=True, path=FUSED, **HOST) as plan:
        assert _nb(plan) == (-1.0, False, -1.0, False)


# ---- the algebra on the emulator -----------------------------------------------------------------------------------------
class NeighbourEmu(FusedEmu):
    """The fused path's emulator with the neighbour form in the dimensions the plan takes it: the carry stages without the
    transfer across a tile (A^L = 0), i.e. c_s0(t) = tau_s0(t), c_s1(t) = tau_s1(t) + W_v(t)[0->1] tau_s0(t-1)."""

    def __init__(self, plan, scans, clamped):
        super().__init__(plan, scans, clamped)
        _, tx, _, ty = _nb(plan)
        if tx:
            self.Ax = np.zeros_like(self.Ax)
        if ty:
            self.Ay = np.zeros_like(self.Ay)


@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3", "BICUBIC_COEFF"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("shape", [(3 * 128 + 1, 2 * 256 + 100), (2 * 128 + 70, 3 * 256)], ids=["short_last_rows", "partial_rows"])
def test_truncated_carry_stages_match_the_full_ones_and_the_oracle(coeff, clamped, shape):
    scans = rc.xy_pm(getattr(rc, coeff))
    img = rc.random_image(shape, np.float32, 61)
    with rfa.Plan(shape, scans, clamped=clamped, path=FUSED, flags=capi.RF_PLAN_TILE_ROWS(128), **HOST) as plan:
        assert plan.tiles[:2] == (256, 128)
        _, tx, _, ty = _nb(plan)
        assert tx and ty
        full = FusedEmu(plan, scans, clamped).run(img)
        nb = NeighbourEmu(plan, scans, clamped).run(img)
    want = oracle.apply_filter(img.astype(np.float64), scans, clamped)
    peak = float(np.max(np.abs(full)))
    assert float(np.max(np.abs(nb - full))) <= 1e-9 * peak          # f64 emulators: what the neighbour form drops is ~1e-12
    assert rc.rel_err(nb, want) < 1e-4


@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3", "BICUBIC_COEFF"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
def test_reported_bound_matches_the_recurrences(coeff, clamped):
    """The bound rf_plan_table("neighbour_carries") reports, x (256 columns) and y (128 rows), against the same quantity formed
    from the recurrences in numpy -- the chaining W of the interior and the last tile included."""
    co = getattr(rc, coeff)
    with rfa.Plan((1024, 2048), rc.xy_pm(co), clamped=clamped, path=FUSED, flags=capi.RF_PLAN_TILE_ROWS(128), **HOST) as plan:
        assert plan.tiles[:2] == (256, 128)
        bx, tx, by, ty = _nb(plan)
        np.testing.assert_allclose(bx, _numpy_bound(co, 256, clamped), rtol=1e-6, atol=0)
        np.testing.assert_allclose(by, _numpy_bound(co, 128, clamped), rtol=1e-6, atol=0)
        assert tx and ty
