"""The cases of the implicit time-accurate driver (fvhip_bdf_device) proved on the host (tests/bdf_host.py: the BDF
equations solved by scipy's Newton-Krylov round the oracle's residual) before any device is asked to meet them, and
the entry points' argument refusals. No GPU.

The figures quoted were measured on the host with f_tol 1e-12 on G*h/area in the max norm.
"""
import ctypes

import numpy as np
import pytest

import fvens_amd._ffi as ffi
import bdf_host as bh
import ssprk_host as sh


# --- coefficients ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [0.3, 1.0, 2.0])
def test_bdf2_coefficients(w):
    """a0 + a1 + a2 = 0, and (a0 p(t1) + a1 p(t0) + a2 p(t-1))/h = p'(t1) for p = 1, t, t^2 on the uneven grid
    t-1 = -h/w, t0 = 0, t1 = h"""
    h = 0.37
    a0, a1, a2 = bh.coefficients(2, 1, h, h / w)
    assert abs(a0 + a1 + a2) <= 4e-16
    if w == 1.0:
        assert (a0, a1, a2) == (1.5, -2.0, 0.5) and a0 + a1 + a2 == 0.0
    tm, t0, t1 = -h / w, 0.0, h
    for p, dp in ((lambda t: 1.0, 0.0), (lambda t: t, 1.0), (lambda t: t * t, 2.0 * t1)):
        assert abs((a0 * p(t1) + a1 * p(t0) + a2 * p(tm)) / h - dp) <= 1e-14


def test_first_step_and_order_one_are_bdf1():
    assert bh.coefficients(1, 5, 0.1, 0.2) == (1.0, -1.0, 0.0)
    assert bh.coefficients(2, 0, 0.1, 0.0) == (1.0, -1.0, 0.0)


# --- temporal order -------------------------------------------------------------------------------------

def _order_errors(order, Ns):
    ref = bh.order_reference()
    return [float(np.abs(bh.host_order_run(order, N)[0] - ref).max()) for N in Ns]


@pytest.mark.parametrize("order", [2, 1])
def test_temporal_order_against_ssprk3(order):
    """ssprk_host.order_case(), T = 1, fixed dt = 1/N; the error is max |u_N - u_ref| against the host SSP-RK3 run
    at N = 256 (its own error is below 1e-6: its step-halving difference, tests/test_ssprk_host.py). Measured:
              N = 32     N = 64     N = 128    N = 256    observed orders
      BDF2    5.93e-3    1.550e-3   3.92e-4    9.84e-5    1.94, 1.98, 2.00
      BDF1    --         2.491e-2   1.310e-2   6.72e-3    0.93, 0.96
    Below N = 32 BDF2 is not yet asymptotic (1.54 from 8 to 16). Asserted: the N = 64 -> 128 order within 0.25 of
    the nominal one, the SSP tests' margin."""
    e64, e128 = _order_errors(order, (64, 128))
    observed = float(np.log2(e64 / e128))
    print(f"BDF{order}: errors N=64 {e64:.4e}, N=128 {e128:.4e}, observed order {observed:.3f}")
    for N in (64, 128):
        _, st, rec = bh.host_order_run(order, N)
        assert st["steps"] == N and st["time"] == sh.ORDER_T
    assert abs(observed - order) <= 0.25, observed


def test_inner_tolerance_is_below_the_temporal_error():
    """the device stops its inner iteration at g <= tol*g0, g = sqrt(sum area sum_v G^2), tol = 1e-8. Solved on the
    host to that test with tol 1e-8 and with tol 5e-9, and to f_tol 1e-12, the N = 128 BDF2 states must differ by
    less than 1 % of the temporal error there (3.92e-4). Measured: tol 1e-8 and 5e-9 give the same state (Newton's
    last step overshoots both), and it differs from the f_tol 1e-12 state by 5.5e-12, 1.4e-8 of the temporal error."""
    ref = bh.order_reference()
    tight = bh.host_order_run(2, 128)[0]
    temporal = float(np.abs(tight - ref).max())
    loose = bh.host_order_run(2, 128, rel_tol=1e-8)[0]
    half = bh.host_order_run(2, 128, rel_tol=5e-9)[0]
    d_half, d_tight = float(np.abs(loose - half).max()), float(np.abs(loose - tight).max())
    print(f"N=128 BDF2: temporal error {temporal:.4e}; tol 1e-8 against 5e-9: {d_half:.3e}, against f_tol 1e-12: "
          f"{d_tight:.3e} ({d_tight / temporal:.2e} of the temporal error)")
    assert d_half < 0.01 * temporal and d_tight < 0.01 * temporal


# --- the vortex beyond the explicit limit ----------------------------------------------------------------

def test_vortex_beyond_the_explicit_limit():
    """vortex_case(16) (256 cells, dtmin 0.0458), BDF2 at fixed dt = 0.2 (h/dtmin = 4.4), ten steps to t = 2.
    Measured: density error 8.883e-3 against the explicit cfl-0.5 run's 8.517e-3 (ratio 1.043: the error is
    spatial); SSP-RK3 at the same dt = 0.2 gives 0.1013; BDF2 at dt = 0.4 gives 1.043e-2. Asserted: BDF2 within 1.1 of
    the explicit error (the margin covers the measured 4 %), and SSP-RK3 at dt = 0.2 at least 5 times it, so the
    case is past what the explicit driver can do."""
    _, st, e_bdf = bh.host_vortex_run(16)
    _, st_x, e_x = sh.host_vortex_run(16)
    b, p, num, u0 = sh.vortex_case(16)
    _, pt = b.physics(sh.VORTEX["Minf"])
    with np.errstate(all="ignore"):
        u_rk, st_rk, _ = sh.ssprk(b.residual(pt, num), b.area, u0, 3, sh.VORTEX["finaltime"], 100, dt=bh.VORTEX_DT)
        e_rk = sh.density_error(b, p, u_rk, st_rk["time"])
    print(f"vortex n=16: BDF2 dt 0.2 {e_bdf:.4e} ({st}), explicit cfl 0.5 {e_x:.4e}, ratio {e_bdf / e_x:.4f}; "
          f"SSP-RK3 at dt 0.2 {e_rk:.4e}")
    assert st["steps"] == 10 and st["time"] == sh.VORTEX["finaltime"]
    assert 4.0 < st["cfl_max"] < 5.0
    assert e_bdf <= 1.1 * e_x
    assert not e_rk < 5.0 * e_x            # at least 5 times, or not finite


# --- refusals: checked before the handle, so they answer without a GPU ---------------------------------

def _call(group, cfg, icfg, stats=True, dstats=True):
    lib = ffi.lib()
    st, ds = ffi.FvUnsteadyStats(), ffi.FvDualTimeStats()
    f = lib.fvhip_group_bdf_device if group else lib.fvhip_bdf_device
    rc = f(None, None, ctypes.byref(cfg) if cfg is not None else None,
           ctypes.byref(icfg) if icfg is not None else None, ctypes.byref(st) if stats else None,
           ctypes.byref(ds) if dstats else None, None)
    return rc, lib.fvhip_last_error().decode()


def _inner(**kw):
    import fvens_amd as fa
    return fa.ImplicitConfig(**kw)._struct()


@pytest.mark.parametrize("group", [False, True])
@pytest.mark.parametrize("fields,inner,msg", [
    (dict(order=3), {}, "BDF: temporal order must be 1 or 2"),
    (dict(order=0), {}, "BDF: temporal order must be 1 or 2"),
    (dict(maxsteps=0), {}, "maxsteps must be >= 1"),
    (dict(finaltime=0.0), {}, "finaltime must be > 0"),
    (dict(finaltime=float("nan")), {}, "finaltime must be > 0"),
    (dict(cfl=0.0, dt=0.0), {}, "BDF: exactly one of cfl > 0 and dt > 0"),
    (dict(cfl=0.5, dt=0.1), {}, "BDF: exactly one of cfl > 0 and dt > 0"),
    ({}, dict(maxiter=0), "maxiter (inner iterations per step) must be >= 1"),
    ({}, dict(resume=(1.0, 0.5, 0.6, 10.0)), "BDF: resume_*"),
])
def test_arguments_refused_by_name(group, fields, inner, msg):
    good = dict(order=2, cfl=0.5, dt=0.0, finaltime=1.0, maxsteps=10)
    good.update(fields)
    rc, err = _call(group, ffi.FvUnsteadyConfig(**good), _inner(**inner))
    assert rc != 0 and msg in err, err


@pytest.mark.parametrize("group", [False, True])
def test_null_pointers_refused(group):
    good = ffi.FvUnsteadyConfig(order=2, cfl=0.5, dt=0.0, finaltime=1.0, maxsteps=10)
    assert _call(group, None, _inner()) == (1, "null config")
    assert _call(group, good, None) == (1, "null implicit config")
    assert _call(group, good, _inner(), stats=False) == (1, "null stats")
    assert _call(group, good, _inner(), dstats=False) == (1, "null dual-time stats")
    assert _call(group, good, _inner()) == (1, "null group" if group else "null handle")
