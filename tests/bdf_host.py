"""Host restatement of the implicit time-accurate driver (fvhip_bdf_device: BDF1/BDF2 in dual time) in numpy and
scipy around the oracle's residual, on the cases of tests/ssprk_host.py.

The residual leaves r = -r(u), so area du/dt = r, and one step of size h from un (and um = u^(n-1)) finds u with
    G(u) = r(u) - (area/h)*((a0*u + a1*un) + a2*um) = 0
BDF1: a = (1, -1, 0). BDF2 with w = h/h_prev: a0 = (1+2w)/(1+w), a1 = -(1+w), a2 = w^2/(1+w); its first step is a
BDF1 step. The step-size bookkeeping is the device's (and ssprk's): h = dt or cfl*dtmin at the step's start state,
set to finaltime - t when t + h >= finaltime or ends within SLIVER*h of it (ten steps of 0.2 sum to 2 - 2^-52; a step
of that remainder has w ~ 1e-15 and the rounding of a0 + a1 dominates its G), and then t = finaltime.

The BDF state is defined by G = 0, whoever solves it. Here that is scipy.optimize.newton_krylov from u = un --
deliberately not the device's pseudo-time iteration -- on F = G*h/area (the state's units) in the max norm, or, with
rel_tol, on G in the device's norm g = sqrt(sum area sum_v G^2) down to rel_tol*g(un): the device's stopping test.
"""
import numpy as np
import scipy.optimize as so

import ssprk_host as sh

F_TOL = 1e-12
SLIVER = 1e-9      # the driver's BDF_SLIVER: a step that ends this close (of itself) to finaltime lands on it


def coefficients(order, step, h, hprev):
    """(a0, a1, a2) of step number `step` (0-based) of a run of the given order"""
    if order == 1 or step == 0:
        return 1.0, -1.0, 0.0
    w = h / hprev
    return (1.0 + 2.0 * w) / (1.0 + w), -(1.0 + w), w * w / (1.0 + w)


def unsteady_residual(r, area, u, un, um, a, h):
    """G in the device kernel's association (k_bdf_residual): bit for bit in float64 without contraction"""
    a0, a1, a2 = a
    d = a0 * u + a1 * un
    if a2 != 0.0:
        d = d + a2 * um
    return r - (area / h)[:, None] * d


def gnorm(G, area):
    """the driver's norm of G: the energy norm's area weighting over all four variables"""
    return float(np.sqrt((area[:, None] * G * G).sum()))


def solve_step(residual, area, un, um, a, h, f_tol=F_TOL, rel_tol=None):
    """u with G(u) = 0 from u = un. Returns (u, residual evaluations)"""
    A = area[:, None]
    count = [0]

    def G(u):
        count[0] += 1
        return unsteady_residual(residual(u)[0], area, u, un, um, a, h)

    if rel_tol is None:
        u = so.newton_krylov(lambda u: G(u) * (h / A), un.copy(), f_tol=f_tol, method="lgmres", maxiter=200)
    else:
        g0 = gnorm(G(un), area)
        if g0 == 0.0:
            return un.copy(), count[0]
        u = so.newton_krylov(G, un.copy(), f_tol=rel_tol * g0, method="lgmres", maxiter=200,
                             tol_norm=lambda x: gnorm(x.reshape(un.shape), area))
    return u, count[0]


def bdf(residual, area, u0, order, finaltime, maxsteps, cfl=0.0, dt=0.0, f_tol=F_TOL, rel_tol=None):
    """residual(u) -> (-r(u), local time steps). Returns (u, stats with the ssprk keys, record [steps][2] = t, h)"""
    assert order in (1, 2) and (cfl > 0) != (dt > 0)
    u, um = u0.copy(), None
    t, step, hprev = 0.0, 0, 0.0
    hs, ratios, rec = [], [], []
    while t < finaltime and step < maxsteps:
        dtmin = residual(u)[1].min()
        if not np.isfinite(dtmin):
            raise RuntimeError("BDF dual time diverged - residual is Nan or inf!")
        h = dt if dt > 0 else cfl * dtmin
        last = t + h >= finaltime or finaltime - (t + h) <= SLIVER * h
        if last:
            h = finaltime - t
        a = coefficients(order, step, h, hprev)
        un = u
        u, _ = solve_step(residual, area, un, um, a, h, f_tol, rel_tol)
        um, hprev = un, h
        t = finaltime if last else t + h
        step += 1
        hs.append(h)
        ratios.append(h / dtmin)
        rec.append([t, h])
    stats = dict(steps=step, time=t, dt_min=min(hs), dt_max=max(hs), cfl_max=max(ratios))
    return u, stats, np.array(rec)


_RUNS = {}


def host_order_run(order, N, rel_tol=None):
    """the order case of ssprk_host integrated to ORDER_T in N fixed BDF steps on the host, computed once"""
    key = ("order", order, N, rel_tol)
    if key not in _RUNS:
        b, p, n, u0, res = sh.order_case()
        _RUNS[key] = bdf(res, b.area, u0, order, sh.ORDER_T, 10 * N, dt=sh.ORDER_T / N, rel_tol=rel_tol)
    return _RUNS[key]


def order_reference():
    """the order case's reference state: the host SSP-RK3 run at N = 256 (its own error is below 1e-6)"""
    return sh.host_order_run(3, 256)[0]


VORTEX_DT = 0.2


def host_vortex_run(n, dt=VORTEX_DT):
    """the vortex of ssprk_host on the n x n box by BDF2 at fixed dt: (u, stats, density error), computed once"""
    key = ("vortex", n, dt)
    if key not in _RUNS:
        b, p, num, u0 = sh.vortex_case(n)
        _, pt = b.physics(sh.VORTEX["Minf"])
        u, st, _ = bdf(b.residual(pt, num), b.area, u0, 2, sh.VORTEX["finaltime"], 100000, dt=dt)
        _RUNS[key] = (u, st, sh.density_error(b, p, u, st["time"]))
    return _RUNS[key]
