"""The implicit time-accurate driver on the device (fvhip_bdf_device, fvhip_group_bdf_device: BDF1/BDF2 in dual
time), its two kernels through their own entry points, and its edges. The BDF state is defined by G(u) = 0, whoever
solves it, so the driver is held to the discrete equation under the oracle's residual and to the temporal order and
the vortex error proved on the host (tests/test_bdf_host.py), not to an iteration count.

Inner tolerance 1e-8 throughout: on the host, solving to it or to 1e-12 moves the N = 128 BDF2 state by 1.4e-8 of
its temporal error (tests/test_bdf_host.py), so nothing tighter is needed.
"""
import math

import numpy as np
import pytest

import fvens_amd as fa
import cases
import bdf_host as bh
import ssprk_host as sh
from test_gpu_residual import get_mesh

pytestmark = pytest.mark.gpu

TOL = 1e-8
# the inner iteration: the pseudo CFL from 1e3 to 1e6 (the physical term a0/h dominates the diagonal from the start),
# linear solves to 1e-3; the cap is far above the iterations measured below
INNER = dict(tol=TOL, maxiter=300, cflinit=1e3, cflfin=1e6, lin_rtol=1e-3, lin_maxit=60, restart=30)


def _torch():
    import torch
    return torch


def _t(a):
    return _torch().tensor(np.ascontiguousarray(a), device="cuda")


def _zeros(*shape):
    return _torch().zeros(shape, dtype=_torch().float64, device="cuda")


def _naca(seed):
    m, om = get_mesh("naca_small")
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    return m, om, p, n, cases.state(m, p, seed)


def _plate(nx, ny):
    m = fa.UMesh.flat_plate(nx, ny)
    return m, cases.physics("plate_inviscid"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")


def _kernel_mesh(name):
    if name == "naca_small":
        m, _, p, n, _ = _naca(1)
        return m, p, n
    if name == "large":
        import gmres_host as gh
        return gh.large_mesh(), cases.physics("naca"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    return _plate(*{"P11": (1, 1), "P255": (15, 17), "P256": (16, 16), "P257": (1, 257)}[name])


def _residual(dev, du, N):
    dr, dt = _zeros(N, 4), _zeros(N)
    _torch().cuda.synchronize()
    dev.compute_residual_device(du.data_ptr(), dr.data_ptr(), dt.data_ptr(), True)
    dev.synchronize()
    return dr.cpu().numpy(), dt.cpu().numpy()


# --- 1. k_bdf_residual against numpy --------------------------------------------------------------------

@pytest.mark.parametrize("name", ["P11", "P255", "P256", "P257", "naca_small", "large"])
def test_bdf_residual_kernel_bitwise(name):
    """fvhip_bdf_residual_device, all in the internal cell order: G bit for bit numpy's
    r - (area/h)*((a0*u + a1*un) + a2*um) for BDF1 (um null), BDF2 at w = 1 and w = 0.37, and G == r for
    u = un = um at w = 1, where a0 + a1 + a2 is exactly 0. That identity needs a0*u exact, so its state is rounded
    to float32 values first: 1.5*u of a full mantissa rounds, and then (1.5u - 2u) + 0.5u is that rounding error,
    not 0. The sum area * sum_v G^2 against math.fsum of the same terms within 1e-12, the project's bar for fixed-tree
    sums of non-negative terms (measured: at most 3e-16). One cell, 255 / 256 / 257 cells (either side
    of one block of the cell kernels), and 294,912 cells (every lane of the partial kernel takes a second trip; a
    skipped trip loses more than half of the sum). On naca_small the residual is bitwise the oracle's."""
    m, p, n = _kernel_mesh(name)
    N = m.nelem
    dev = fa.FlowFV(m, p, n)
    perm = dev.permutation()
    area = np.ascontiguousarray(m.area[:N][perm])
    u, un, um = (np.ascontiguousarray(cases.state(m, p, s)[perm]) for s in (11, 12, 13))
    u32 = u.astype(np.float32).astype(np.float64)
    _, dtm = _residual(dev, _t(u), N)
    h = 20.0 * dtm.min()
    worst = 0.0
    for label, (uu, nn, mm), a in (("bdf1", (u, un, None), (1.0, -1.0, 0.0)),
                                   ("bdf2 w=1", (u, un, um), bh.coefficients(2, 1, h, h)),
                                   ("bdf2 w=0.37", (u, un, um), bh.coefficients(2, 1, h, h / 0.37)),
                                   ("identity", (u32, u32, u32), bh.coefficients(2, 1, h, h))):
        du, dn, dg = _t(uu), _t(nn), _zeros(N, 4)
        dm = _t(mm) if mm is not None else None
        r, _ = _residual(dev, du, N)
        sumsq = dev.bdf_residual_device(du.data_ptr(), dn.data_ptr(), dm.data_ptr() if mm is not None else None,
                                        *a, h, dg.data_ptr())
        G = dg.cpu().numpy()
        ref = bh.unsteady_residual(r, area, uu, nn, mm, a, h)
        np.testing.assert_array_equal(G, ref, err_msg=label)
        if label == "identity":
            assert a[0] + a[1] + a[2] == 0.0
            np.testing.assert_array_equal(G.view(np.uint64), r.view(np.uint64))
        else:
            assert np.abs(G - r).max() > 0
        terms = area * (((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2]) + G[:, 3] * G[:, 3])
        exact = math.fsum(terms)
        worst = max(worst, abs(sumsq - exact) / exact)
        assert abs(sumsq - exact) <= 1e-12 * exact, (label, sumsq, exact)
    print(f"{name} ({N} cells): sum area*G^2 against fsum, worst relative difference {worst:.2e}")
    if name == "naca_small":
        _, om, _, _, _ = _naca(1)
        r_dev, _ = _residual(dev, _t(u), N)
        u_ref = np.empty_like(u)
        u_ref[perm] = u
        np.testing.assert_array_equal(r_dev, sh.oracle_residual(om, p, n)(u_ref)[0][perm])
    dev.close()


# --- 2. k_bdf_time_term ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["P11", "P257", "naca_small"])
def test_time_term_kernel_bitwise(name):
    """after assemble_jacobian_device + add_pseudo_time_term_device, add_physical_time_term_device(s) leaves
    d_mdt and the four diagonal entries of every block numpy's x + s*area bit for bit, the twelve other entries and
    the face blocks as they were; a residual and its time steps afterwards are bitwise what they were before"""
    m, p, n = _kernel_mesh(name)
    N, Fi = m.nelem, max(m.naface - m.nbface, 1)
    dev = fa.FlowFV(m, p, n)
    perm = dev.permutation()
    area = np.ascontiguousarray(m.area[:N][perm])
    du = _t(cases.state(m, p, 14)[perm])
    r0, dt0 = _residual(dev, du, N)
    dd, dl, dup, dmdt = _zeros(N, 16), _zeros(Fi, 16), _zeros(Fi, 16), _t(dt0)
    _torch().cuda.synchronize()
    dev.assemble_jacobian_device(du.data_ptr(), dd.data_ptr(), dl.data_ptr(), dup.data_ptr())
    dev.add_pseudo_time_term_device(50.0, dmdt.data_ptr(), dd.data_ptr())
    dev.synchronize()
    before = [x.cpu().numpy() for x in (dd, dl, dup, dmdt)]
    s = 1.5 / (20.0 * dt0.min())
    dev.add_physical_time_term_device(s, dmdt.data_ptr(), dd.data_ptr())
    dev.synchronize()
    after = [x.cpu().numpy() for x in (dd, dl, dup, dmdt)]
    want = before[0].copy()
    want[:, [0, 5, 10, 15]] = before[0][:, [0, 5, 10, 15]] + (s * area)[:, None]
    np.testing.assert_array_equal(after[0], want)
    np.testing.assert_array_equal(after[3], before[3] + s * area)
    assert (after[3] > before[3]).all()
    np.testing.assert_array_equal(after[1], before[1])
    np.testing.assert_array_equal(after[2], before[2])
    r1, dt1 = _residual(dev, du, N)
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(dt1, dt0)
    dev.close()


# --- 3., 4. the returned state satisfies the discrete equation under the oracle ------------------------------

def _run_one(m, p, n, u0, cfg, *args, **kw):
    """one handle on the whole mesh: (state in reference order, stats, record)"""
    dev = fa.FlowFV(m, p, n)
    perm = dev.permutation()
    du = _t(u0[perm])
    _torch().cuda.synchronize()
    st, rec = dev.bdf_device(du.data_ptr(), *args, cfg, record=True, **kw)
    u = np.empty_like(u0)
    u[perm] = du.cpu().numpy()
    dev.close()
    return u, st, rec


def _run_group(m, p, n, u0, cfg, *args, nranks=3, **kw):
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
    torch.cuda.synchronize()
    grp = fa.FlowFVGroup(sps)
    try:
        st, rec = grp.bdf_device([d.data_ptr() for d in dus], *args, cfg, record=True, **kw)
        u = np.full_like(u0, np.nan)
        for k, sp in enumerate(sps):
            u[glob[k]] = dus[k][:sp.nown].cpu().numpy()
    finally:
        grp.close()
        for sp in sps:
            sp.close()
    return u, st, rec


def _oracle_ratio(res, area, u, un, um, a, h):
    """g(u)/g(un) of the step's unsteady residual under the oracle: what the driver's test saw, in numpy's order"""
    g1 = bh.gnorm(bh.unsteady_residual(res(u)[0], area, u, un, um, a, h), area)
    g0 = bh.gnorm(bh.unsteady_residual(res(un)[0], area, un, un, um, a, h), area)
    return g1 / g0


def _check_two_steps(run, label):
    m, om, p, n, u0 = _naca(21)
    res, area = sh.oracle_residual(om, p, n), np.ascontiguousarray(m.area[:m.nelem])
    h = 20.0 * float(res(u0)[1].min())
    u1, st1, rec1 = run(m, p, n, u0, 2, 1e9, 1, dt=h)
    u2, st2, rec2 = run(m, p, n, u0, 2, 1e9, 2, dt=h)
    assert st1["steps"] == 1 and st2["steps"] == 2 and st2["time"] == 2 * h
    assert st1["inner_unconverged"] == 0 and st2["inner_unconverged"] == 0
    assert 0 < st2["inner_max"] < INNER["maxiter"] and st2["worst_ratio"] <= TOL
    np.testing.assert_array_equal(rec2[0], rec1[0])              # deterministic: the first step again
    q1 = _oracle_ratio(res, area, u1, u0, None, (1.0, -1.0, 0.0), h)
    q2 = _oracle_ratio(res, area, u2, u1, u0, bh.coefficients(2, 1, h, h), h)
    print(f"{label}: inner iterations per step {rec2[:, 2]}, Krylov {st2['lin_iters']} (unconverged solves "
          f"{st2['lin_unconverged']}); g/g0 device {rec2[:, 3]}, oracle {q1:.3e} {q2:.3e}; cfl_max {st2['cfl_max']:.2f}")
    assert np.abs(u1 - u0).max() > 1e-4 and np.abs(u2 - u1).max() > 1e-4
    assert q1 <= 1.01 * TOL and q2 <= 1.01 * TOL
    return u1, u2


@pytest.mark.parametrize("prec", ["jacobi", "lines"])
@pytest.mark.parametrize("matrix_free", [False, True])
def test_state_satisfies_the_bdf_equation(matrix_free, prec):
    """naca_small, perturbed free stream, BDF2 at dt = 20 dtmin(u0), one step and then two from the same start: the
    second run's first step is the first run's bitwise, and under the oracle's residual g(u1)/g(u0) of the BDF1
    start and g(u2)/g(u1) of the BDF2 step are within 1.01 of the inner tolerance (the 1 % covers numpy's summation
    order against the device's tree), with no step at the cap. Iterations per step are printed, not asserted"""
    cfg = fa.ImplicitConfig(matrix_free=matrix_free, prec_lines=(prec == "lines"), **INNER)
    u1, _ = _check_two_steps(lambda m, p, n, u0, *a, **kw: _run_one(m, p, n, u0, cfg, *a, **kw),
                             f"matrix_free={matrix_free} {prec}")
    # the two-step run's first step is seen through its record row (iterations, g/g0, the four sums: equal bits
    # above); the one-step run again, on a new handle, gives the state's bits
    m, _, p, n, u0 = _naca(21)
    again, _, _ = _run_one(m, p, n, u0, cfg, 2, 1e9, 1, dt=_H21())
    np.testing.assert_array_equal(again, u1)


def _H21():
    m, om, p, n, u0 = _naca(21)
    return 20.0 * float(sh.oracle_residual(om, p, n)(u0)[1].min())


def test_group_satisfies_the_bdf_equation():
    """the same case on a 3-rank in-process group, gathered: the same oracle check. The group adds the ranks' partial
    sums on the host, so its norms and Krylov coefficients are not one handle's bits; the difference of the states is
    printed, not asserted"""
    cfg = fa.ImplicitConfig(**INNER)
    u1, u2 = _check_two_steps(lambda m, p, n, u0, *a, **kw: _run_group(m, p, n, u0, cfg, *a, **kw), "group of 3")
    m, _, p, n, u0 = _naca(21)
    one, _, _ = _run_one(m, p, n, u0, cfg, 2, 1e9, 2, dt=_H21())
    print(f"group against one handle after two steps: max |du| {np.abs(u2 - one).max():.3e} "
          f"(the steps moved the state by {np.abs(one - u0).max():.3e})")


# --- 5. temporal order on the periodic handle ---------------------------------------------------------------

_PERIODIC = {}


def periodic_bdf(b, p, n, u0, cfg, *args, **kw):
    """the driver on the periodic handle of box b, ghost rows NaN before: (state, stats, record)"""
    torch = _torch()
    m = b.P
    sp = fa.FlowFV(m, p, n)
    perm = sp.permutation()
    d = torch.full((m.nelem + m.nconnface, 4), float("nan"), dtype=torch.float64, device="cuda")
    d[:m.nelem] = torch.tensor(np.ascontiguousarray(u0[perm]), device="cuda")
    torch.cuda.synchronize()
    st, rec = sp.bdf_device(d.data_ptr(), *args, cfg, record=True, **kw)
    u = np.empty_like(u0)
    u[perm] = d[:m.nelem].cpu().numpy()
    sp.close()
    return u, st, rec


@pytest.mark.parametrize("order", [2, 1])
def test_temporal_order_on_device(order):
    """the host order case on the periodic handle: N = 64 and 128 fixed steps to T = 1, errors max |u_N - u_ref|
    against the device's own SSP-RK3 run at N = 256; the observed order within 0.25 of the nominal one. Host figures
    (tests/test_bdf_host.py): BDF2 1.550e-3, 3.92e-4 (1.98); BDF1 2.491e-2, 1.310e-2 (0.93). Device: the same to the
    digits printed"""
    from test_gpu_ssprk import device_order_run
    b, p, n, u0, _ = sh.order_case()
    ref, st_ref, _ = device_order_run(3, 256)
    assert st_ref["time"] == sh.ORDER_T
    cfg = fa.ImplicitConfig(**INNER)
    err, inner = [], []
    for N in (64, 128):
        u, st, rec = periodic_bdf(b, p, n, u0, cfg, order, sh.ORDER_T, 10 * N, dt=sh.ORDER_T / N)
        assert st["steps"] == N and st["time"] == sh.ORDER_T and st["inner_unconverged"] == 0
        err.append(float(np.abs(u - ref).max()))
        inner.append(st["inner_iters"] / N)
    observed = float(np.log2(err[0] / err[1]))
    print(f"device BDF{order}: errors N=64 {err[0]:.4e}, N=128 {err[1]:.4e}, observed order {observed:.3f}; "
          f"inner iterations per step {inner}")
    assert abs(observed - order) <= 0.25, observed


# --- 6. vortex ----------------------------------------------------------------------------------------------

def test_vortex_beyond_the_explicit_limit():
    """vortex_case(16), BDF2 at dt = 0.2 (4.4 dtmin): ten steps land on t = 2 and the density error is within 1.1
    of the device's own cfl-0.5 SSP-RK3 error (host: 8.883e-3 against 8.517e-3)"""
    from test_gpu_ssprk import periodic_run
    b, p, num, u0 = sh.vortex_case(16)
    ux, stx, _ = periodic_run(b, p, num, u0, sh.VORTEX["order"], sh.VORTEX["finaltime"], 100000, cfl=sh.VORTEX["cfl"])
    e_x = sh.density_error(b, p, ux, stx["time"])
    u, st, rec = periodic_bdf(b, p, num, u0, fa.ImplicitConfig(**INNER), 2, sh.VORTEX["finaltime"], 100, dt=bh.VORTEX_DT)
    e = sh.density_error(b, p, u, st["time"])
    print(f"vortex n=16 on the device: BDF2 dt 0.2 {e:.4e} in {st['steps']} steps (inner {rec[:, 2]}), "
          f"SSP-RK3 cfl 0.5 {e_x:.4e} in {stx['steps']} steps, ratio {e / e_x:.4f}; cfl_max {st['cfl_max']:.2f}")
    assert st["time"] == sh.VORTEX["finaltime"] and st["steps"] == 10 and st["inner_unconverged"] == 0
    assert e <= 1.1 * e_x


# --- 7. final-time landing ----------------------------------------------------------------------------------

def test_final_time_landing():
    """three steps at fixed dt, finaltime 0.1 % past the third: a fourth step of h = finaltime - t3 exactly lands on
    it, and that cut step (w = h/dt != 1) satisfies the variable-step equation under the oracle"""
    m, om, p, n, u0 = _naca(22)
    res, area = sh.oracle_residual(om, p, n), np.ascontiguousarray(m.area[:m.nelem])
    cfg = fa.ImplicitConfig(**INNER)
    dt = 20.0 * float(res(u0)[1].min())
    t3 = dt + dt + dt
    final = t3 * 1.001
    us = {k: _run_one(m, p, n, u0, cfg, 2, final, k, dt=dt)[0] for k in (2, 3)}
    u4, st, rec = _run_one(m, p, n, u0, cfg, 2, final, 100, dt=dt)
    assert st["steps"] == 4 and st["time"] == final and rec.shape == (4, 8)
    assert rec[2, 0] == t3 and rec[3, 0] == final and rec[3, 1] == final - t3
    assert (rec[:3, 1] == dt).all() and st["dt_min"] == final - t3 < 0.01 * st["dt_max"]
    h4 = final - t3
    q = _oracle_ratio(res, area, u4, us[3], us[2], bh.coefficients(2, 3, h4, dt), h4)
    print(f"cut step: w = {h4 / dt:.3e}, inner {rec[3, 2]:.0f}, g/g0 device {rec[3, 3]:.3e}, oracle {q:.3e}")
    assert st["inner_unconverged"] == 0 and q <= 1.01 * TOL


def test_cfl_mode_takes_the_hosts_step():
    """cfl mode: h = cfl * dtmin of the step's start state, the oracle's bits on naca_small"""
    m, om, p, n, u0 = _naca(22)
    dtmin = float(sh.oracle_residual(om, p, n)(u0)[1].min())
    _, st, rec = _run_one(m, p, n, u0, fa.ImplicitConfig(**INNER), 2, 1e9, 1, cfl=20.0)
    assert st["steps"] == 1 and rec[0, 1] == 20.0 * dtmin and st["time"] == rec[0, 0] == 20.0 * dtmin
    assert st["cfl_max"] == (20.0 * dtmin) / dtmin


# --- 8. edges ----------------------------------------------------------------------------------------------

def test_free_stream_takes_no_iteration():
    """the free stream at zero incidence on the uniform 8 x 8 quadrangle box (spacing 1.25, exact in binary): every
    variable's flux is carried by one pair of opposite faces with exactly opposite normals, so the residual is
    exactly zero (the oracle's on the tiling is) and g0 = 0: no inner iteration, the state bitwise unchanged, a final
    ratio of 0 (no 0/0). BDF1 steps see G = r - q*(u - u) = r for any state. A BDF2 step with u = un = um sees
    G = r - q*((1.5u - 2u) + 0.5u), which is r only where 1.5*u is exact: the free stream's energy 7.642857... has a
    full mantissa, 1.5 E rounds, and G is that rounding error times area/h. So the BDF2 run takes the uniform state
    rounded to float32 values (no boundary on the box: every uniform state is steady).
    Where g0 is rounding instead of 0 -- BDF2 on the unrounded free stream (seen: the two BDF2 steps ran their 300
    iterations), an incidence, the jittered boxes (|r| 1e-16 to 1e-14) -- the relative test cannot be met and the
    step runs to the cap: DESIGN 6d, not built."""
    b = sh.box(8, 8, "quad", jitter=0.0)
    p, _ = b.physics(0.5)
    p.aoa = 0.0
    n = cases.numerics("ROE", "LEASTSQUARES", "NONE")
    free = np.ascontiguousarray(np.tile(cases.freestream(p), (b.P.nelem, 1)))
    for order, u0 in ((1, free), (2, free.astype(np.float32).astype(np.float64))):
        u, st, rec = periodic_bdf(b, p, n, u0, fa.ImplicitConfig(**INNER), order, 1.0, 3, dt=0.1)
        print(f"uniform state, order {order}: {st}")
        assert st["steps"] == 3 and st["inner_iters"] == 0 and st["worst_ratio"] == 0.0
        assert (rec[:, 2] == 0).all() and (rec[:, 3] == 0).all() and np.isfinite(rec).all()
        np.testing.assert_array_equal(u.view(np.uint64), u0.view(np.uint64))


def test_nan_in_one_cell_diverges():
    m, _, p, n, u0 = _naca(23)
    u0[m.nelem // 3, 0] = np.nan
    cfg = fa.ImplicitConfig(**INNER)
    for kw in (dict(cfl=20.0), dict(dt=1e-4)):
        with pytest.raises(RuntimeError, match="BDF dual time diverged - residual is Nan or inf!"):
            _run_one(m, p, n, u0, cfg, 2, 1e9, 2, **kw)
    with pytest.raises(RuntimeError, match="BDF dual time diverged - residual is Nan or inf!"):
        _run_group(m, p, n, u0, cfg, 2, 1e9, 2, cfl=20.0)


def test_refusals_leave_the_handle_working():
    m, _, p, n, u0 = _naca(24)
    dev = fa.FlowFV(m, p, n)
    du = _t(u0[dev.permutation()])
    r0, dt0 = _residual(dev, du, m.nelem)
    good = fa.ImplicitConfig(**INNER)
    with pytest.raises(RuntimeError, match="BDF: temporal order must be 1 or 2"):
        dev.bdf_device(du.data_ptr(), 3, 1.0, 10, good, cfl=5.0)
    with pytest.raises(RuntimeError, match=r"BDF: resume_\*"):
        dev.bdf_device(du.data_ptr(), 2, 1.0, 10, fa.ImplicitConfig(resume=(1.0, 0.5, 0.6, 10.0), **INNER), cfl=5.0)
    with pytest.raises(RuntimeError, match="BDF: exactly one of cfl > 0 and dt > 0"):
        dev.bdf_device(du.data_ptr(), 2, 1.0, 10, good, cfl=5.0, dt=1e-3)
    with pytest.raises(RuntimeError, match="BDF: exactly one of cfl > 0 and dt > 0"):
        dev.bdf_device(du.data_ptr(), 2, 1.0, 10, good)
    with pytest.raises(RuntimeError, match="null u"):
        dev.bdf_device(None, 2, 1.0, 10, good, cfl=5.0)
    np.testing.assert_array_equal(du.cpu().numpy(), u0[dev.permutation()])     # nothing was stepped
    r1, dt1 = _residual(dev, du, m.nelem)
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(dt1, dt0)
    dev.close()


def test_one_cell_takes_two_steps():
    """flat_plate(1, 1): no interior face, one block of one live lane; two BDF2 steps stay finite"""
    m, p, n = _plate(1, 1)
    u0 = cases.state(m, p, 25)
    u, st, rec = _run_one(m, p, n, u0, fa.ImplicitConfig(**INNER), 2, 1e9, 2, cfl=5.0)
    print(f"one cell: {st}, record {rec}")
    assert st["steps"] == 2 and np.isfinite(u).all() and np.isfinite(rec).all()
