"""Host restatement of the time-accurate SSP Runge-Kutta driver (fvhip_ssprk_device) in numpy around the
oracle's residual, the periodic boxes it is tested on, and the isentropic vortex.

The loop is the device's, operation for operation (float64, no contraction), so on a mesh where the device
residual is bitwise the oracle's the integrator is too:
    r, dtm = -r(u), local time steps;  dtmin = min dtm;  h = dt if dt > 0 else cfl*dtmin
    if t + h >= finaltime: h = finaltime - t, and t = finaltime after the step; else t += h
    stage s: us = (c0*u + c1*us) + ((c2*h)/area)*r, with r taken at us for s >= 2;  the last stage is the new u

The oracle has no periodicity. For a periodic box P the state is replicated onto the 3 x 3 tiling T of P (far
field round T) and the residual and time steps are read at the centre tile, again at every stage
(tests/test_gpu_periodic.py's Case does that once): the stencil reaches two cells, the tile is at least eight wide.
"""
import os
import tempfile

import numpy as np

import fvens_amd as fa
import _oracle as orc
import cases
import periodic_meshes as pmesh

COEF = {1: [(1.0, 0.0, 1.0)],
        2: [(1.0, 0.0, 1.0), (0.5, 0.5, 0.5)],
        3: [(1.0, 0.0, 1.0), (0.75, 0.25, 0.25), (0.3333333333333333, 0.6666666666666667, 0.6666666666666667)]}


def ssprk(residual, area, u0, order, finaltime, maxsteps, cfl=0.0, dt=0.0, stage_state=True):
    """residual(u) -> (-r(u), local time steps). Returns (u, stats as the device's, record [steps][6]).
    stage_state=False: every stage's residual at the step's start state, as the reference's TVDRKSolver::solve
    passes it (aodesolver.cpp:719) -- the sign corrected, everything else the same."""
    assert (cfl > 0) != (dt > 0)
    A = area[:, None]
    u = u0.copy()
    t, step = 0.0, 0
    hs, ratios, rec = [], [], []
    while t < finaltime and step < maxsteps:
        r, dtm = residual(u)
        dtmin = dtm.min()
        if not np.isfinite(dtmin):
            raise RuntimeError("SSP-RK diverged - dtmin is Nan or inf!")
        h = dt if dt > 0 else cfl * dtmin
        last = t + h >= finaltime
        if last:
            h = finaltime - t
        us = u
        for s, (c0, c1, c2) in enumerate(COEF[order]):
            if s > 0 and stage_state:
                r, _ = residual(us)
            us = (c0 * u + c1 * us) + ((c2 * h) / A) * r
        u = us
        t = finaltime if last else t + h
        step += 1
        hs.append(h)
        ratios.append(h / dtmin)
        rec.append([t, h] + list((u * A).sum(axis=0)))
    stats = dict(steps=step, time=t, dt_min=min(hs), dt_max=max(hs), cfl_max=max(ratios))
    return u, stats, np.array(rec)


def oracle_residual(om, p, n):
    """residual(u) of one oracle mesh"""
    ref = orc.OracleSpatial(om, p, n)
    N = om.nelem

    def residual(u):
        r, dtm = np.zeros((N, 4)), np.zeros(N)
        ref.compute_residual(np.ascontiguousarray(u), r, True, dtm)
        return r, dtm
    return residual


_DIR = None
_BOXES = {}
_RUNS = {}


def _workdir():
    global _DIR
    if _DIR is None:
        _DIR = tempfile.TemporaryDirectory(prefix="ssprk_boxes_")
    return _DIR.name


class Box:
    """the doubly periodic nx x ny box P of side lx x ly and its 3 x 3 tiling T for the oracle"""

    def __init__(self, nx, ny, kind, lx, ly, jitter):
        tag = f"{nx}x{ny}{kind}"
        pp, tp = os.path.join(_workdir(), f"P{tag}.msh"), os.path.join(_workdir(), f"T{tag}.msh")
        pmesh.write_tiling(pp, nx, ny, kind, 1, 1, lx, ly, jitter, markers=(5, 4, 5, 4))
        tile, self.local = pmesh.write_tiling(tp, nx, ny, kind, 3, 3, lx, ly, jitter, markers=(9, 9, 9, 9))
        self.P = fa.UMesh.read_gmsh(pp).periodic([(4, 0), (5, 1)])
        self.oT = orc.OracleMesh.read(tp)
        self.centre = np.nonzero((tile[:, 0] == 1) & (tile[:, 1] == 1))[0]
        np.testing.assert_array_equal(self.local[self.centre], np.arange(self.P.nelem))
        self.lx, self.ly = lx, ly
        self.area = np.ascontiguousarray(self.P.area[:self.P.nelem])
        self.rc = np.ascontiguousarray(self.P.rc[:self.P.nelem])

    def physics(self, Minf=0.5):
        """(physics on P: no boundary at all; on T: the far field round the tiling)"""
        p, t = cases.physics("naca", Minf=Minf), cases.physics("naca", Minf=Minf)
        p.bcconf = []
        t.bcconf = [fa.FlowBCConfig("farfield", 9)]
        return p, t

    def residual(self, pt, n):
        ref = orc.OracleSpatial(self.oT, pt, n)
        NT = self.oT.nelem

        def residual(u):
            r, dtm = np.zeros((NT, 4)), np.zeros(NT)
            ref.compute_residual(np.ascontiguousarray(u[self.local]), r, True, dtm)
            return r[self.centre], dtm[self.centre]
        return residual


def box(nx, ny, kind, lx=10.0, ly=10.0, jitter=0.2):
    key = (nx, ny, kind, lx, ly, jitter)
    if key not in _BOXES:
        _BOXES[key] = Box(*key)
    return _BOXES[key]


def smooth_numerics():
    """HLLC + least squares + unlimited linear reconstruction: smooth in the state, so that step halving sees
    the integrator's order. Roe's entropy-fix kinks and Van Albada make the third-order ratios erratic
    (1.0 to 3.4 on the same box)."""
    return cases.numerics("HLLC", "LEASTSQUARES", "NONE")


def order_case():
    """the temporal-order case: hybrid 8 x 8 box (96 cells), side 10, jitter 0.2, smooth state, M 0.5.
    Returns (box, physics on P, numerics, u0, residual)"""
    b = box(8, 8, "hybrid")
    p, pt = b.physics(0.5)
    n = smooth_numerics()
    u0 = pmesh.smooth_state(b.rc, p, lx=b.lx, ly=b.ly, seed=3)
    if "order_residual" not in _RUNS:
        _RUNS["order_residual"] = b.residual(pt, n)
    return b, p, n, u0, _RUNS["order_residual"]


ORDER_T = 1.0
ORDER_N = (16, 32, 64, 128, 256)


def halving_orders(finals):
    """observed orders log2(e_k / e_k+1), e_k = max |u_N - u_2N|, of the final states for N, 2N, 4N, ..."""
    e = [np.abs(a - b).max() for a, b in zip(finals[:-1], finals[1:])]
    return [float(np.log2(a / b)) for a, b in zip(e[:-1], e[1:])], e


def host_order_run(order, N, stage_state=True):
    """the order case integrated to ORDER_T in N fixed steps on the host, computed once"""
    key = ("order", order, N, stage_state)
    if key not in _RUNS:
        b, p, n, u0, res = order_case()
        _RUNS[key] = ssprk(res, b.area, u0, order, ORDER_T, 10 * N, dt=ORDER_T / N, stage_state=stage_state)
    return _RUNS[key]


# --- the isentropic vortex ----------------------------------------------------------------------------

VORTEX = dict(strength=5.0, order=3, cfl=0.5, finaltime=2.0, Minf=0.5)


def vortex(rc, p, t, lx=10.0, ly=10.0, strength=5.0):
    """conserved state at the points rc of the isentropic vortex of the given strength that started at the box
    centre and is carried by the free stream (rho 1, velocity (cos aoa, sin aoa), p = 1/(gamma M^2)) for time t,
    wrapped over the lx x ly box (each point sees the nearest image of the centre). With T = p/rho:
    dv = strength/(2 pi) exp((1 - r^2)/2) (-y, x), dT = -(gamma-1) strength^2/(8 gamma pi^2) exp(1 - r^2),
    rho = (T/Tinf)^(1/(gamma-1)), p = rho T: an exact solution of the Euler equations."""
    g, M, a = p.gamma, p.Minf, p.aoa
    Tinf = 1.0 / (g * M * M)
    vx0, vy0 = np.cos(a), np.sin(a)
    dx = np.mod(rc[:, 0] - (0.5 * lx + vx0 * t) + 0.5 * lx, lx) - 0.5 * lx
    dy = np.mod(rc[:, 1] - (0.5 * ly + vy0 * t) + 0.5 * ly, ly) - 0.5 * ly
    r2 = dx * dx + dy * dy
    f = strength / (2 * np.pi) * np.exp(0.5 * (1 - r2))
    vx, vy = vx0 - f * dy, vy0 + f * dx
    T = Tinf - (g - 1) * strength ** 2 / (8 * g * np.pi ** 2) * np.exp(1 - r2)
    rho = (T / Tinf) ** (1.0 / (g - 1))
    pr = rho * T
    u = np.empty((rc.shape[0], 4))
    u[:, 0] = rho
    u[:, 1] = rho * vx
    u[:, 2] = rho * vy
    u[:, 3] = pr / (g - 1) + 0.5 * rho * (vx * vx + vy * vy)
    return np.ascontiguousarray(u)


def density_error(b, p, u, t):
    """area-weighted L2 error of the density against the exact vortex at time t"""
    exact = vortex(b.rc, p, t, b.lx, b.ly, VORTEX["strength"])
    return float(np.sqrt(((u[:, 0] - exact[:, 0]) ** 2 * b.area).sum() / b.area.sum()))


def vortex_case(n):
    """(box, physics on P, numerics, u0) of the vortex on the n x n quadrangle box"""
    b = box(n, n, "quad")
    p, _ = b.physics(VORTEX["Minf"])
    return b, p, smooth_numerics(), vortex(b.rc, p, 0.0, b.lx, b.ly, VORTEX["strength"])


def host_vortex_run(n):
    """the vortex on the n x n box integrated on the host: (u, stats, density error), computed once"""
    key = ("vortex", n)
    if key not in _RUNS:
        b, p, num, u0 = vortex_case(n)
        _, pt = b.physics(VORTEX["Minf"])
        u, st, _ = ssprk(b.residual(pt, num), b.area, u0, VORTEX["order"], VORTEX["finaltime"], 100000,
                         cfl=VORTEX["cfl"])
        _RUNS[key] = (u, st, density_error(b, p, u, st["time"]))
    return _RUNS[key]
