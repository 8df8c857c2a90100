"""The cases of the time-accurate SSP Runge-Kutta driver proved on the host (tests/ssprk_host.py around the
oracle's residual) before any device is asked to meet them, and the entry points' argument refusals. No GPU.

Numerics of the order and vortex cases: HLLC + least squares + unlimited linear reconstruction. Step halving
measures the integrator only if the residual is smooth in the state; Roe's entropy-fix kinks and Van Albada make
the third-order ratios erratic (1.0 to 3.4 on the same box), HLLC with the unlimited reconstruction does not.
"""
import copy
import ctypes

import numpy as np
import pytest

import fvens_amd._ffi as ffi
import ssprk_host as sh


@pytest.mark.parametrize("order", [1, 2, 3])
def test_temporal_order_by_step_halving(order):
    """hybrid 8 x 8 periodic box (96 cells, side 10), smooth state, M 0.5, fixed dt = 1/N for N = 16 ... 256:
    e_k = max |u_N - u_2N|, observed order log2(e_k / e_k+1). Measured (three successive ratios):
    order 1: 1.39 1.22 1.11, order 2: 2.010 2.013 2.010, order 3: 2.989 3.009 3.007. The last two are the
    asymptotic range and must lie within 0.25 of the nominal order (the margin covers the first-order scheme's
    slow approach, 1.22). The largest step is 1.25 dtmin, stable for all three orders."""
    runs = [sh.host_order_run(order, N) for N in sh.ORDER_N]
    assert [st["steps"] for _, st, _ in runs] == list(sh.ORDER_N)
    assert all(st["time"] == sh.ORDER_T for _, st, _ in runs)
    assert 1.2 < runs[0][1]["cfl_max"] < 1.3
    orders, e = sh.halving_orders([u for u, _, _ in runs])
    print(f"order {order}: differences {e}, observed orders {orders}")
    assert all(abs(o - order) <= 0.25 for o in orders[-2:]), orders


def test_reference_loop_is_first_order():
    """the reason the driver exists: the reference's loop takes every stage's residual at the step's start
    state (aodesolver.cpp:719), and with the Shu-Osher coefficients that is forward Euler. "Order 3" of that loop
    (sign corrected) measures 1.39 1.22 1.11, the first-order scheme's ratios, and its final states are forward
    Euler's to rounding."""
    fin = [sh.host_order_run(3, N, stage_state=False)[0] for N in sh.ORDER_N]
    orders, e = sh.halving_orders(fin)
    print(f"reference loop, order 3: differences {e}, observed orders {orders}")
    assert all(o < 1.5 for o in orders[-2:]), orders
    euler = [sh.host_order_run(1, N)[0] for N in sh.ORDER_N]
    assert max(np.abs(a - b).max() for a, b in zip(fin, euler)) <= 1e-12 * np.abs(euler[0]).max()


def test_vortex_against_exact_solution():
    """isentropic vortex of strength 5 on the 10 x 10 periodic quadrangle box, order 3, cfl 0.5, to t = 2:
    the area-weighted L2 density error against the exact solution falls by at least 2 from n = 16 to n = 32 (a
    condition: at least first order with room to spare; measured 8.52e-3 and 2.05e-3, ratio 4.2), and the run
    lands on the final time exactly."""
    (_, s16, e16), (_, s32, e32) = sh.host_vortex_run(16), sh.host_vortex_run(32)
    print(f"vortex: n=16 {s16} error {e16:.4e}; n=32 {s32} error {e32:.4e}; ratio {e16 / e32:.3f}")
    assert s16["time"] == sh.VORTEX["finaltime"] and s32["time"] == sh.VORTEX["finaltime"]
    assert s16["cfl_max"] <= sh.VORTEX["cfl"] and s32["cfl_max"] <= sh.VORTEX["cfl"]
    assert e16 / e32 >= 2.0


def test_vortex_is_a_steady_solution_in_its_frame():
    """the exact solution used above: at t = 0 the vortex sits at the box centre, far from it the state is the free
    stream, and after one period of the carrying stream along x the wrapped vortex is back where it was"""
    b, p, _, u0 = sh.vortex_case(16)
    centre = np.argmin(np.hypot(b.rc[:, 0] - 5.0, b.rc[:, 1] - 5.0))
    assert u0[centre, 0] == u0[:, 0].min() < 0.9
    corner = np.argmax(np.hypot(b.rc[:, 0] - 5.0, b.rc[:, 1] - 5.0))
    assert abs(u0[corner, 0] - 1.0) < 1e-6
    p0 = copy.copy(p)
    p0.aoa = 0.0
    np.testing.assert_allclose(sh.vortex(b.rc, p0, 10.0), sh.vortex(b.rc, p0, 0.0), rtol=0, atol=1e-13)


def test_tvdrk_stage_is_the_rk_stage_with_negated_step():
    """ode.hip has one stage kernel, k_rk_stage: out = (c0*u + c1*us) + (sc/area)*r. The TVD-RK driver, whose
    stage the reference writes c0*u + c1*us - (sc/area)*r (aodesolver.cpp:735-744), calls it with -sc. The two are
    the same bits because (-sc)/area = -(sc/area), (-t)*r = -(t*r) and a + (-x) = a - x are exact in IEEE-754
    (the kernel is built without contraction, as numpy evaluates here). 1e6 seeded rows whose every operand is
    drawn from ordinary values, signed zeros, infinities, subnormals, the extremes of the range and values that
    make the sum cancel; every Shu-Osher (c0, c1) and random ones. Byte for byte, except that where one side is
    NaN the other must be NaN too (a NaN's sign is not part of the claim)."""
    rng = np.random.default_rng(20240607)
    n = 1_000_000
    tiny = np.finfo(np.float64).tiny
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, tiny / 8, -tiny / 8, tiny, -tiny,
                        np.finfo(np.float64).max, -np.finfo(np.float64).max, 1.0, -1.0])

    def draw(positive=False):
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-12, 13, n)
        k = rng.random(n) < 0.3
        x[k] = special[rng.integers(0, len(special), k.sum())]
        return np.abs(x) if positive else x

    stages = np.array([(1.0, 0.0), (0.5, 0.5), (0.75, 0.25), (0.3333333333333333, 0.6666666666666667)])
    c = stages[rng.integers(0, len(stages), n)]
    k = rng.random(n) < 0.2
    c[k] = rng.standard_normal((k.sum(), 2))
    c0, c1 = c[:, 0], c[:, 1]
    u, us, r, sc, area = draw(), draw(), draw(), draw(), draw(positive=True)
    # rows that cancel: t*r equal to the sum it is subtracted from, exactly or to the last bits
    k = rng.random(n) < 0.2
    with np.errstate(all="ignore"):
        r[k] = ((c0 * u + c1 * us) / (sc / area))[k] * rng.choice([1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53], k.sum())
        written = c0 * u + c1 * us - (sc / area) * r            # k_tvdrk_stage's expression, as the reference has it
        called = (c0 * u + c1 * us) + ((-sc) / area) * r        # k_rk_stage with the step negated
    nan = np.isnan(written)
    assert np.array_equal(nan, np.isnan(called))
    assert 0.05 * n < nan.sum() < 0.9 * n                       # the specials reach both kinds of row
    assert np.count_nonzero(written == 0.0) > 1000 and np.count_nonzero(np.isinf(written)) > 1000
    same = written.view(np.uint64) == called.view(np.uint64)
    assert np.all(same | nan), f"{np.count_nonzero(~(same | nan))} rows differ"


# --- refusals: checked before the handle, so they answer without a GPU ---------------------------------

def _call(group, cfg, stats=True, handle=None):
    lib = ffi.lib()
    st = ffi.FvUnsteadyStats()
    f = lib.fvhip_group_ssprk_device if group else lib.fvhip_ssprk_device
    rc = f(handle, None, ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(st) if stats else None, None)
    return rc, lib.fvhip_last_error().decode()


@pytest.mark.parametrize("group", [False, True])
@pytest.mark.parametrize("fields,msg", [
    (dict(order=0), "temporal order must be 1, 2 or 3"),
    (dict(order=4), "temporal order must be 1, 2 or 3"),
    (dict(maxsteps=0), "maxsteps must be >= 1"),
    (dict(finaltime=0.0), "finaltime must be > 0"),
    (dict(finaltime=-1.0), "finaltime must be > 0"),
    (dict(finaltime=float("nan")), "finaltime must be > 0"),
    (dict(cfl=0.0, dt=0.0), "exactly one of cfl > 0 and dt > 0"),
    (dict(cfl=0.5, dt=0.1), "exactly one of cfl > 0 and dt > 0"),
    (dict(cfl=-0.5, dt=float("nan")), "exactly one of cfl > 0 and dt > 0"),
])
def test_arguments_refused_by_name(group, fields, msg):
    good = dict(order=3, cfl=0.5, dt=0.0, finaltime=1.0, maxsteps=10)
    good.update(fields)
    rc, err = _call(group, ffi.FvUnsteadyConfig(**good))
    assert rc != 0 and msg in err, err


@pytest.mark.parametrize("group", [False, True])
def test_null_pointers_refused(group):
    good = ffi.FvUnsteadyConfig(order=3, cfl=0.5, dt=0.0, finaltime=1.0, maxsteps=10)
    assert _call(group, None) == (1, "null config")
    assert _call(group, good, stats=False) == (1, "null stats")
    # a good configuration reaches the handle check
    assert _call(group, good) == (1, "null group" if group else "null handle")
