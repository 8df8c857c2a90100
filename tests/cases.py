"""Shared test cases: meshes (reference fixtures + synthetic), configurations mirroring the
reference's control files, and seeded flow states."""
import os

import numpy as np

import fvens_amd as fa
from fvens_amd import FlowBCConfig, FlowNumericsConfig, FlowPhysicsConfig

HERE = os.path.dirname(os.path.abspath(__file__))
MESHDIR = os.path.join(HERE, "fixtures", "meshes")


def fixture_mesh(name):
    return os.path.join(MESHDIR, name + ".msh")


def physics(kind, aoa_deg=0.0, Minf=None):
    """Physics + BCs of the reference test decks.
    'cyl'   inviscid cylinder, tests/inv-2dcyl/inv-cyl-base.ctrl (slipwall 2, farfield 4, M 0.38)
    'naca'  transonic NACA0012, testcases/naca0012/transonic-sanity-test-muscl.ctrl (M 0.8, 1.25 deg)
    'visc'  laminar NACA0012, testcases/visc-naca0012/laminar-implicit.ctrl (Re 5000, M 0.5, alpha 0: :19-31)
    'plate' flat plate, tests/visc-flatplate/flatplate.ctrl (M 0.2, Re 8.7e5, T 290.19 K, Pr 0.708)
    'wall'  tests/flow-general/test.ctrl (farfield 4, adiabatic 2, isothermal 3; M 0.5, Re 5000);
            the deck's wall temperature 290 is used as a non-dimensional value by abc.cpp:349-366,
            which makes the ghost state non-physical, so 1.1 (x free-stream T) is used here
    """
    d2r = np.pi / 180.0
    if kind == "cyl":
        return FlowPhysicsConfig(gamma=1.4, Minf=Minf or 0.38, aoa=aoa_deg * d2r,
                                 bcconf=[FlowBCConfig("slipwall", 2), FlowBCConfig("farfield", 4)])
    if kind == "naca":
        return FlowPhysicsConfig(gamma=1.4, Minf=Minf or 0.8, aoa=1.25 * d2r,
                                 bcconf=[FlowBCConfig("slipwall", 2), FlowBCConfig("farfield", 4)])
    if kind == "visc":
        return FlowPhysicsConfig(gamma=1.4, Minf=Minf or 0.5, Tinf=288.15, Reinf=5000.0, Pr=0.72,
                                 aoa=aoa_deg * d2r, viscous_sim=True,
                                 bcconf=[FlowBCConfig("adiabaticwall", 2, [0.0]),
                                         FlowBCConfig("inflowoutflow", 4)])
    if kind == "viscconst":
        p = physics("visc")
        p.const_visc = True
        return p
    if kind == "plate":
        return FlowPhysicsConfig(gamma=1.4, Minf=Minf or 0.2, Tinf=290.19, Reinf=8.7e5, Pr=0.708,
                                 viscous_sim=True,
                                 bcconf=[FlowBCConfig("slipwall", 3), FlowBCConfig("adiabaticwall", 2, [0.0]),
                                         FlowBCConfig("farfield", 4), FlowBCConfig("inflowoutflow", 5)])
    if kind == "plate_inviscid":
        return FlowPhysicsConfig(gamma=1.4, Minf=Minf or 0.2,
                                 bcconf=[FlowBCConfig("slipwall", 3), FlowBCConfig("extrapolation", 2),
                                         FlowBCConfig("farfield", 4), FlowBCConfig("inflowoutflow", 5)])
    if kind == "wall":
        return FlowPhysicsConfig(gamma=1.4, Minf=0.5, Tinf=288.15, Reinf=5000.0, Pr=0.72, viscous_sim=True,
                                 bcconf=[FlowBCConfig("farfield", 4), FlowBCConfig("adiabaticwall", 2, [0.0]),
                                         FlowBCConfig("isothermalwall", 3, [0.0, 1.1])])
    raise ValueError(kind)


def numerics(flux="ROE", grad="LEASTSQUARES", rec="VANALBADA", order2=True, jac=None, K=20.0):
    return FlowNumericsConfig(conv_numflux=flux, conv_numflux_jac=jac or flux, gradientscheme=grad,
                              reconstruction=rec, limiter_param=K, order2=order2)


def freestream(p):
    g, M, a = p.gamma, p.Minf, p.aoa
    pinf = 1.0 / (g * M * M)
    return np.array([1.0, np.cos(a), np.sin(a), pinf / (g - 1.0) + 0.5])


def state(mesh, p, seed=42, amp=0.05):
    """Free stream perturbed smoothly: rho, p *(1+amp sin), v += amp sin, seeded."""
    rng = np.random.default_rng(seed)
    x = mesh.rc[:mesh.nelem, 0]
    y = mesh.rc[:mesh.nelem, 1]
    g, M, a = p.gamma, p.Minf, p.aoa
    pinf = 1.0 / (g * M * M)

    def wave():
        k = rng.integers(1, 5, size=2)
        ph = rng.random(2)
        return np.sin(2 * np.pi * (k[0] * x / 3.0 + ph[0])) * np.cos(2 * np.pi * (k[1] * y / 3.0 + ph[1]))
    rho = 1.0 * (1 + amp * wave())
    pr = pinf * (1 + amp * wave())
    vx = np.cos(a) + amp * wave()
    vy = np.sin(a) + amp * wave()
    u = np.empty((mesh.nelem, 4))
    u[:, 0] = rho
    u[:, 1] = rho * vx
    u[:, 2] = rho * vy
    u[:, 3] = pr / (g - 1.0) + 0.5 * rho * (vx * vx + vy * vy)
    return np.ascontiguousarray(u)


REGIME_MACH = (2.0, 2.0, 0.0, 0.3, 0.6, 1.0)


def regime_state(mesh_or_rc, p, seed, jump=1.4):
    """Piecewise-smooth state that puts every flow regime on one mesh: six angular sectors about the
    centroid of the cell centres, the sector boundaries rotated by a seeded angle.
      sector 0  M 2 along +x        1  M 2 along -x        2  exactly at rest (velocities stored as 0.0)
             3  M 0.3 radially out  4  M 0.6 radially in   5  M 1 tangential (counter-clockwise)
    rho is 1 or `jump` alternating by sector, p is pinf or 1.2 jump pinf alternating by sector pairs, the
    speed is M sqrt(gamma p/rho) of the cell; rho, p and the speed each carry a 1 + 0.03 sin cos wave with
    seeded wavenumbers 1..3 over the mesh extent. Supersonic faces of both signs, sonic lines, cells at
    rest and jumps in every variable (limiters clip) follow; pure numpy, deterministic in (rc, p, seed).
    mesh_or_rc: anything with .rc and .nelem, or the [nelem][2] array of cell centres."""
    if hasattr(mesh_or_rc, "rc"):
        rc = np.asarray(mesh_or_rc.rc, np.float64)[:mesh_or_rc.nelem]
    else:
        rc = np.asarray(mesh_or_rc, np.float64)
    rng = np.random.default_rng(seed)
    x, y = rc[:, 0], rc[:, 1]
    g, M = p.gamma, p.Minf
    pinf = 1.0 / (g * M * M)
    dx, dy = x - x.mean(), y - y.mean()
    rad = np.maximum(np.hypot(dx, dy), 1e-300)
    rot = 2 * np.pi * rng.random()
    sec = np.minimum((np.mod(np.arctan2(dy, dx) - rot, 2 * np.pi) / (np.pi / 3)).astype(np.int64), 5)
    x0, y0 = x.min(), y.min()
    lx, ly = max(x.max() - x0, 1e-300), max(y.max() - y0, 1e-300)

    def wave():
        k = rng.integers(1, 4, size=2)
        ph = rng.random(2)
        return 1 + 0.03 * (np.sin(2 * np.pi * (k[0] * (x - x0) / lx + ph[0])) *
                           np.cos(2 * np.pi * (k[1] * (y - y0) / ly + ph[1])))
    rho = np.where(sec % 2 == 0, 1.0, jump) * wave()
    pr = np.where((sec // 2) % 2 == 0, pinf, 1.2 * jump * pinf) * wave()
    speed = np.asarray(REGIME_MACH)[sec] * np.sqrt(g * pr / rho) * wave()
    ex, ey = dx / rad, dy / rad
    dirx = np.choose(sec, [1.0, -1.0, 0.0, ex, -ex, -ey])
    diry = np.choose(sec, [0.0, 0.0, 0.0, ey, -ey, ex])
    vx = np.where(sec == 2, 0.0, speed * dirx)
    vy = np.where(sec <= 2, 0.0, speed * diry)
    u = np.empty((rc.shape[0], 4))
    u[:, 0] = rho
    u[:, 1] = np.where(sec == 2, 0.0, rho * vx)
    u[:, 2] = np.where(sec <= 2, 0.0, rho * vy)
    u[:, 3] = pr / (g - 1.0) + 0.5 * rho * (vx * vx + vy * vy)
    return np.ascontiguousarray(u)


def sonic_faces(nf=200, seed=5, g=1.4):
    """Face states at the kinks of Roe's entropy fix: the normal velocity is c (s + e) with s in {0, 1, -1}
    and e = +-5e-5, so the Roe-averaged |vn|, |vn - c| or |vn + c| lies inside Harten's delta = 1e-4 c; every
    other face has ur == ul, the others ur one relative 1e-6 step away from ul (a non-zero jump, so the fixed
    eigenvalue reaches the flux). Returns ul, ur, n and the number of faces that take each of the three fix
    lines (|vn - c|, |vn|, |vn + c| < delta on the Roe average, anumericalflux.cpp:686-692), in numpy."""
    rng = np.random.default_rng(seed)
    k = np.arange(nf)
    s = np.array([0.0, 1.0, -1.0])[k % 3]
    e = np.where((k // 3) % 2 == 0, 5e-5, -5e-5)
    rho = 1 + 0.3 * rng.random(nf)
    pr = (1 + 0.3 * rng.random(nf)) / (g * 0.64)
    c = np.sqrt(g * pr / rho)
    th = 2 * np.pi * rng.random(nf)
    n = np.stack([np.cos(th), np.sin(th)], 1)
    vn, vt = c * (s + e), 0.7 * rng.standard_normal(nf)
    vx, vy = vn * n[:, 0] - vt * n[:, 1], vn * n[:, 1] + vt * n[:, 0]
    ul = np.stack([rho, rho * vx, rho * vy, pr / (g - 1) + 0.5 * rho * (vx * vx + vy * vy)], 1)
    step = np.where(((k // 6) % 2 == 1)[:, None], 1e-6 * rng.uniform(-1, 1, (nf, 4)), 0.0)
    ur = ul * (1 + step)

    def vars_(u):
        v = u[:, 1:3] / u[:, :1]
        p = (g - 1) * (u[:, 3] - 0.5 * u[:, 0] * (v * v).sum(1))
        return v, (u[:, 3] + p) / u[:, 0]
    vi, Hi = vars_(ul)
    vj, Hj = vars_(ur)
    R = np.sqrt(ur[:, 0] / ul[:, 0])
    va = (R[:, None] * vj + vi) / (R[:, None] + 1)
    ca = np.sqrt((g - 1) * ((R * Hj + Hi) / (R + 1) - 0.5 * (va * va).sum(1)))
    vna = (va * n).sum(1)
    hits = [int(np.sum(np.abs(vna - ca) < 1e-4 * ca)), int(np.sum(np.abs(vna) < 1e-4 * ca)),
            int(np.sum(np.abs(vna + ca) < 1e-4 * ca))]
    return np.ascontiguousarray(ul), np.ascontiguousarray(ur), np.ascontiguousarray(n), hits
