"""The time-accurate SSP Runge-Kutta driver on the device (fvhip_ssprk_device, fvhip_group_ssprk_device)
against its host restatement (tests/ssprk_host.py): bit for bit where the device residual is bitwise the
oracle's (one domain, 3 ranks in process), to the periodic handle's 1e-12 against the oracle's tiling, with the
temporal order measured by step halving, conservation from the record, and the vortex against the exact
solution. The cases and their bars are proved on the host in tests/test_ssprk_host.py.
"""
import numpy as np
import pytest

import fvens_amd as fa
import cases
import ssprk_host as sh
from test_gpu_residual import get_mesh

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _dev(u, perm):
    return _torch().tensor(np.ascontiguousarray(u[perm]), device="cuda")


def _naca(seed):
    m, om = get_mesh("naca_small")
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    return m, om, p, n, cases.state(m, p, seed)


def _run_one(m, p, n, u0, *args, **kw):
    """one handle on the whole mesh: (state in reference order, stats, record)"""
    dev = fa.FlowFV(m, p, n)
    perm = dev.permutation()
    du = _dev(u0, perm)
    _torch().cuda.synchronize()
    st, rec = dev.ssprk_device(du.data_ptr(), *args, **kw)
    u = np.empty_like(u0)
    u[perm] = du.cpu().numpy()
    dev.close()
    return u, st, rec


def _group(m, p, n, u0, nranks=3):
    """(group, handles, per-rank device states with NaN ghost rows, per-rank global cell numbers)"""
    torch = _torch()
    part = fa.partition_graph(m, nranks, weights="cost")
    sps = [fa.FlowFV(m, p, n, partition=part, rank=k) for k in range(nranks)]
    dus, glob = [], []
    for k, sp in enumerate(sps):
        g = np.nonzero(part == k)[0][sp.permutation()]
        glob.append(g)
        d = torch.full((sp.nown + sp.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
        d[:sp.nown] = torch.tensor(u0[g], device="cuda")
        dus.append(d)
    torch.cuda.synchronize()  # torch's stream vs the library's (non-blocking) streams
    return fa.FlowFVGroup(sps), sps, dus, glob


def _close(grp, sps):
    grp.close()
    for sp in sps:
        sp.close()


# --- 1. bitwise against the host loop -----------------------------------------------------------------

@pytest.mark.parametrize("order", [1, 2, 3])
def test_bitwise_vs_host(order):
    m, om, p, n, u0 = _naca(5)
    u_ref, st_ref, rec_ref = sh.ssprk(sh.oracle_residual(om, p, n), m.area[:m.nelem], u0, order, 1e9, 6, cfl=0.4)
    u, st, rec = _run_one(m, p, n, u0, order, 1e9, 6, cfl=0.4, record=True)
    assert st["steps"] == st_ref["steps"] == 6 and rec.shape == (6, 6)
    assert st["time"] == st_ref["time"]
    np.testing.assert_array_equal(rec[:, :2], rec_ref[:, :2])
    np.testing.assert_array_equal(u, u_ref)
    assert (st["dt_min"], st["dt_max"], st["cfl_max"]) == (st_ref["dt_min"], st_ref["dt_max"], st_ref["cfl_max"])
    assert np.abs(u - u0).max() > 1e-6            # the steps moved the state
    # the record's sums against numpy's (another summation order): rounding of a sum of ~7000 terms
    size = (np.abs(u_ref) * m.area[:m.nelem, None]).sum(axis=0)
    assert (np.abs(rec[:, 2:] - rec_ref[:, 2:]) <= 1e-12 * size).all()


# --- 2. final-time landing ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["cfl", "dt"])
def test_final_time_landing(mode):
    """finaltime 0.1 % past the third step's time: a fourth step of h = finaltime - t3 lands on it exactly"""
    m, om, p, n, u0 = _naca(6)
    res, area = sh.oracle_residual(om, p, n), m.area[:m.nelem]
    kw = dict(cfl=0.4)
    if mode == "dt":
        kw = dict(dt=0.4 * res(u0)[1].min())
    _, st3, rec3 = sh.ssprk(res, area, u0, 2, 1e9, 3, **kw)
    t3 = st3["time"]
    final = t3 * 1.001
    u_ref, st_ref, rec_ref = sh.ssprk(res, area, u0, 2, final, 100, **kw)
    u, st, rec = _run_one(m, p, n, u0, 2, final, 100, record=True, **kw)
    assert st["steps"] == st_ref["steps"] == 4
    assert st["time"] == final and st_ref["time"] == final
    assert rec[2, 0] == t3 and rec[3, 0] == final and rec[3, 1] == final - t3
    assert st["dt_min"] == final - t3 < 0.01 * st["dt_max"]
    np.testing.assert_array_equal(rec[:, :2], rec_ref[:, :2])
    np.testing.assert_array_equal(u, u_ref)


# --- 3. group ------------------------------------------------------------------------------------------

def test_group_bitwise_one_handle():
    """3 ranks in one process: the global dtmin and the one-GPU residuals at every stage, so the same bits;
    the stage state's ghost rows are filled by the stage residual's own exchange"""
    m, _, p, n, u0 = _naca(7)
    u1, st1, rec1 = _run_one(m, p, n, u0, 3, 1e9, 4, cfl=0.4, record=True)
    grp, sps, dus, glob = _group(m, p, n, u0)
    st, rec = grp.ssprk_device([d.data_ptr() for d in dus], 3, 1e9, 4, cfl=0.4, record=True)
    u = np.full_like(u0, np.nan)
    for k, sp in enumerate(sps):
        u[glob[k]] = dus[k][:sp.nown].cpu().numpy()
    _close(grp, sps)
    assert st["steps"] == st1["steps"] == 4 and st["time"] == st1["time"]
    np.testing.assert_array_equal(rec[:, :2], rec1[:, :2])
    np.testing.assert_array_equal(u, u1)
    # three partial sums added on the host against one handle's tree: rounding
    size = (np.abs(u1) * m.area[:m.nelem, None]).sum(axis=0)
    assert (np.abs(rec[:, 2:] - rec1[:, 2:]) <= 1e-12 * size).all()


# --- 4.-6. the periodic box: tiling equivalence, temporal order, conservation ----------------------------

_DEVICE_RUNS = {}


def periodic_run(b, p, n, u0, *args, **kw):
    """the driver on the periodic handle of box b, ghost rows NaN before: (state, stats, record)"""
    torch = _torch()
    m = b.P
    sp = fa.FlowFV(m, p, n)
    perm = sp.permutation()
    d = torch.full((m.nelem + m.nconnface, 4), float("nan"), dtype=torch.float64, device="cuda")
    d[:m.nelem] = torch.tensor(np.ascontiguousarray(u0[perm]), device="cuda")
    torch.cuda.synchronize()
    st, rec = sp.ssprk_device(d.data_ptr(), *args, **kw)
    u = np.empty_like(u0)
    u[perm] = d[:m.nelem].cpu().numpy()
    sp.close()
    return u, st, rec


def device_order_run(order, N):
    """the order case in N fixed steps on the periodic handle, with the record, run once"""
    key = (order, N)
    if key not in _DEVICE_RUNS:
        b, p, n, u0, _ = sh.order_case()
        _DEVICE_RUNS[key] = periodic_run(b, p, n, u0, order, sh.ORDER_T, 10 * N, dt=sh.ORDER_T / N, record=True)
    return _DEVICE_RUNS[key]


def test_periodic_handle_equals_tiling():
    """order 3, 16 steps of dt = 1/16 on the 96-cell hybrid box against the host loop on the 3 x 3 tiling. The
    periodic handle's residuals equal the tiling's to ~1e-14, not bitwise, so the bar is that file's
    1e-12 of each variable's max |u|. Measured: 1.6e-15, 1.4e-15, 1.2e-14, 6.7e-16 of max |u| for the four
    variables."""
    u_ref, st_ref, rec_ref = sh.host_order_run(3, 16)
    u, st, rec = device_order_run(3, 16)
    assert st["steps"] == st_ref["steps"] == 16 and st["time"] == st_ref["time"] == sh.ORDER_T
    np.testing.assert_array_equal(rec[:, :2], rec_ref[:, :2])        # fixed dt: the times are the host's bits
    err = np.abs(u - u_ref).max(axis=0) / np.abs(u_ref).max(axis=0)
    print(f"periodic handle against the tiling loop, 16 steps of order 3: {err} of max|u|; "
          f"cfl_max {st['cfl_max']:.6f} (host {st_ref['cfl_max']:.6f})")
    assert np.abs(u - sh.order_case()[3]).max() > 1e-3             # the state moved
    assert (err <= 1e-12).all(), err
    assert abs(st["cfl_max"] - st_ref["cfl_max"]) <= 1e-12 * st_ref["cfl_max"]


@pytest.mark.parametrize("order", [1, 2, 3])
def test_temporal_order_on_device(order):
    """the step-halving runs and bars of tests/test_ssprk_host.py on the periodic handle: the last two observed
    orders within 0.25 of the nominal one. Measured on the device: 1.39 1.22 1.11, 2.010 2.013 2.010,
    2.989 3.009 3.007 -- the host's"""
    runs = [device_order_run(order, N) for N in sh.ORDER_N]
    assert [st["steps"] for _, st, _ in runs] == list(sh.ORDER_N)
    assert all(st["time"] == sh.ORDER_T for _, st, _ in runs)
    orders, e = sh.halving_orders([u for u, _, _ in runs])
    print(f"device, order {order}: differences {e}, observed orders {orders}")
    assert all(abs(o - order) <= 0.25 for o in orders[-2:]), orders


def test_conservation_from_the_record():
    """no boundary and one global step: the four integrals sum area*u stay put to rounding (a face pair is two
    faces evaluated with local normals, |sum r| / sum |r| <= 2e-16, so not exactly). Their size is sum area*|u|,
    the scale of the reduction's own rounding (an integral may cancel, its rounding does not); the bar 1e-12 of
    it over the 16 steps, from the first row to every later one and from the initial state's sums (numpy) to the
    first. Measured drift: at most 9.9e-16 of the size, first row 3.3e-16."""
    b, p, n, u0, _ = sh.order_case()
    u, st, rec = device_order_run(3, 16)
    assert rec.shape == (16, 6)
    size = (np.abs(u0) * b.area[:, None]).sum(axis=0)
    start = (u0 * b.area[:, None]).sum(axis=0)
    drift = np.abs(rec[:, 2:] - rec[0, 2:]).max(axis=0) / size
    first = np.abs(rec[0, 2:] - start) / size
    print(f"conservation over 16 steps: drift {drift}, first row against the initial sums {first} of sum area*|u|")
    assert (drift <= 1e-12).all() and (first <= 1e-12).all()
    # and the record's last row is the returned state's sums
    assert (np.abs(rec[-1, 2:] - (u * b.area[:, None]).sum(axis=0)) <= 1e-12 * size).all()


# --- 7. vortex ------------------------------------------------------------------------------------------

def test_vortex_on_device():
    """n = 16 and n = 32 periodic quadrangle handles against the exact solution: the density error falls by at
    least 2, and each error is within 1e-9 relative of the host restatement's (the states differ by the periodic
    handle's 1e-14 per residual). Measured: 8.517e-3 and 2.050e-3, ratio 4.16, the host's to all digits printed"""
    err = {}
    for nn in (16, 32):
        b, p, num, u0 = sh.vortex_case(nn)
        _, st_ref, e_ref = sh.host_vortex_run(nn)
        u, st, _ = periodic_run(b, p, num, u0, sh.VORTEX["order"], sh.VORTEX["finaltime"], 100000, cfl=sh.VORTEX["cfl"])
        err[nn] = sh.density_error(b, p, u, st["time"])
        print(f"vortex n={nn}: {st}, density error {err[nn]:.6e} (host {e_ref:.6e}, {st_ref['steps']} steps)")
        assert st["time"] == sh.VORTEX["finaltime"] and st["steps"] == st_ref["steps"]
        assert abs(err[nn] - e_ref) <= 1e-9 * e_ref
    assert err[16] / err[32] >= 2.0


# --- 8. divergence and refusals -------------------------------------------------------------------------

def test_nan_in_one_cell_diverges():
    """a NaN density in one cell makes its time step NaN, which the minimum carries: the divergence error, on one
    handle and on the 3-rank group with the NaN on one rank only"""
    m, _, p, n, u0 = _naca(8)
    u0[m.nelem // 3, 0] = np.nan
    one = fa.FlowFV(m, p, n)
    du = _dev(u0, one.permutation())
    _torch().cuda.synchronize()
    for kw in (dict(cfl=0.4), dict(dt=1e-6)):          # the minimum is read in fixed-dt mode too
        with pytest.raises(RuntimeError, match="SSP-RK diverged - dtmin is Nan or inf!"):
            one.ssprk_device(du.data_ptr(), 3, 1e9, 4, **kw)
    one.close()
    grp, sps, dus, _ = _group(m, p, n, u0)
    with pytest.raises(RuntimeError, match="SSP-RK diverged - dtmin is Nan or inf!"):
        grp.ssprk_device([d.data_ptr() for d in dus], 3, 1e9, 4, cfl=0.4)
    _close(grp, sps)


def test_refusals_on_a_handle():
    m, _, p, n, u0 = _naca(9)
    one = fa.FlowFV(m, p, n)
    du = _dev(u0, one.permutation())
    _torch().cuda.synchronize()
    with pytest.raises(RuntimeError, match="temporal order must be 1, 2 or 3"):
        one.ssprk_device(du.data_ptr(), 4, 1.0, 10, cfl=0.4)
    with pytest.raises(RuntimeError, match="exactly one of cfl > 0 and dt > 0"):
        one.ssprk_device(du.data_ptr(), 3, 1.0, 10, cfl=0.4, dt=1e-3)
    with pytest.raises(RuntimeError, match="null u"):
        one.ssprk_device(None, 3, 1.0, 10, cfl=0.4)
    np.testing.assert_array_equal(du.cpu().numpy(), u0[one.permutation()])     # nothing was stepped
    one.close()
