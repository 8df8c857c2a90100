"""High-precision restatement of the two output functionals, in numpy's np.longdouble, written from the
reference's text and independent of the oracle's C++:

  surface_rows(mesh, p, u, grads, marker)   FlowFV_base::computeSurfaceData (flow_spatial.cpp:130-310), with
                                            Sutherland's viscosity from aphysics_defs.hpp:408-421
  entropy_terms(mesh, p, u)                 FlowOutput::compute_entropy_cell (aoutput.cpp:28-62)

Both take the mesh's stored doubles (face normals and lengths, face centres, cell areas) and the state as exact
inputs and carry every operation after that in long double (64-bit mantissa on x86). Sums are math.fsum of the long
double terms rounded to double: the terms then carry a relative 2^-53 each and the sum none. tests/
test_functionals_host.py pins both against the oracle on the CPU.
"""
import math

import numpy as np

LD = np.longdouble
SUTHERLAND_C = LD(110.5)        # IdealGasPhysics::sC (aphysics.cpp:19)


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def marker_faces(mesh, marker):
    """boundary-face indices of `marker`, ascending (the reference's loop order, flow_spatial.cpp:156-158)"""
    return np.nonzero(np.asarray(mesh.btags).reshape(mesh.nbface, -1)[:, 0] == marker)[0]


def wind(p):
    """flowDirectionVector(aoa) with zero side-slip (mathutils.hpp:67-75), in long double from the double angle"""
    a = LD(p.aoa)
    return np.array([np.cos(a) * np.cos(LD(0)), np.sin(a) * np.cos(LD(0))], dtype=LD)


def pressure(p, uc):
    """getPressureFromConserved (aphysics_defs.hpp:60-63) of rows of conserved states"""
    g = LD(p.gamma)
    return (g - 1) * (uc[:, 3] - LD(0.5) * (uc[:, 1] * uc[:, 1] + uc[:, 2] * uc[:, 2]) / uc[:, 0])


def viscosity(p, uc):
    """getViscosityCoeffFromConserved (aphysics_defs.hpp:408-421): Sutherland's law over Re_inf; T^1.5 as T sqrt(T),
    both correctly rounded in long double. Re_inf = inf (inviscid decks) gives exactly 0."""
    g, M, Tinf, Re = LD(p.gamma), LD(p.Minf), LD(p.Tinf), LD(p.Reinf)
    T = pressure(p, uc) / uc[:, 0] * g * M * M                      # getTemperature (:119-122)
    s = SUTHERLAND_C / Tinf
    return (1 + s) / (T + s) * (T * np.sqrt(T)) / Re


def surface_rows(mesh, p, u, grads, marker):
    """per face of `marker`, ascending boundary-face index: rows (x, y, Cp, Cf) and products
    (Cp n.nw len, Cp n.w len, Cf t.w len, len), both [n][4] long double. grads is [nelem][4 vars][2 dims].
    The stress is gradu + gradu^T (:244), so Cf does not depend on which way round the velocity-gradient tensor is
    stored; it does depend on the layout of the gradient block and on the sign of the tangent."""
    faces = marker_faces(mesh, marker)
    le = np.asarray(mesh.intfac)[faces, 0]
    fm = _ld(np.asarray(mesh.facemetric)[faces])
    n, length = fm[:, :2], fm[:, 2]
    tang = np.stack([n[:, 1], -n[:, 0]], 1)                          # n x k (:164-166)
    uc = _ld(np.asarray(u)[le])
    g = _ld(np.asarray(grads).reshape(-1, 4, 2)[le])                 # g[:, var, dim] = grad[lelem](dim, var)
    pinf = 1 / (LD(p.gamma) * LD(p.Minf) * LD(p.Minf))               # getFreestreamPressure (:465-467)
    cp = (pressure(p, uc) - pinf) * 2                                # :205
    mu = viscosity(p, uc)                                            # :226
    rho = uc[:, 0]
    gradu = np.empty((len(faces), 2, 2), dtype=LD)                   # gradu[i][j] = d v_i / d x_j (:229-233)
    for i in range(2):
        for j in range(2):
            gradu[:, i, j] = (g[:, i + 1, j] * rho - uc[:, i + 1] * g[:, 0, j]) / (rho * rho)
    force = np.zeros((len(faces), 2), dtype=LD)                      # :239-247
    for i in range(2):
        for j in range(2):
            force[:, i] += (gradu[:, i, j] + gradu[:, j, i]) * n[:, j]
    tauw = mu * (force[:, 0] * tang[:, 0] + force[:, 1] * tang[:, 1])   # :252
    cf = 2 * tauw                                                    # :255
    w = wind(p)
    nw = np.array([-w[1], w[0]], dtype=LD)                           # flownormal (:150-151)
    ndotw = n[:, 0] * w[0] + n[:, 1] * w[1]
    ndotnw = n[:, 0] * nw[0] + n[:, 1] * nw[1]
    tdotw = tang[:, 0] * w[0] + tang[:, 1] * w[1]
    gr = _ld(np.asarray(mesh.gr).reshape(-1, 2)[faces])
    rows = np.stack([gr[:, 0], gr[:, 1], cp, cf], 1)
    prods = np.stack([cp * ndotnw * length, cp * ndotw * length, cf * tdotw * length, length], 1)   # :292-295
    return rows, prods


def fsum(x):
    """exactly rounded sum of the terms rounded to double, as a long double"""
    return LD(math.fsum(float(v) for v in np.asarray(x).ravel()))


def surface_functionals(prods):
    """(CL, CDp, CDsf) from surface_rows' products (:302-307); 0/0 = NaN for a marker without faces, as the reference"""
    tot = fsum(prods[:, 3])
    with np.errstate(invalid="ignore", divide="ignore"):
        return tuple(fsum(prods[:, k]) / tot for k in range(3))


def freestream(p):
    """compute_freestream_state (aphysics.cpp:43-58)"""
    g, M, a = LD(p.gamma), LD(p.Minf), LD(p.aoa)
    pinf = 1 / (g * M * M)
    return np.array([[LD(1), np.cos(a), np.sin(a), pinf / (g - 1) + LD(0.5)]], dtype=LD)


def entropy_terms(mesh, p, u):
    """per cell ((s - s_inf)/s_inf)^2 area, s = p/rho^gamma (getEntropyFromConserved, aphysics_defs.hpp:204-207)"""
    g = LD(p.gamma)
    uinf = freestream(p)
    sinf = (pressure(p, uinf) / uinf[:, 0] ** g)[0]
    uc = _ld(np.asarray(u)[:mesh.nelem])
    serr = (pressure(p, uc) / uc[:, 0] ** g - sinf) / sinf
    return serr * serr * _ld(np.asarray(mesh.area)[:mesh.nelem])


def entropy_error(mesh, p, u):
    return np.sqrt(fsum(entropy_terms(mesh, p, u)))
