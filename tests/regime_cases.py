"""The regime cases: which (mesh, BC layout, scheme, seed) the GPU regime tests run on cases.regime_state,
and the numpy census of the branches each case is there to reach. One list for test_gpu_regimes.py and
test_regime_cases_host.py (the CPU test that proves the oracle finite and the branches hit for every case),
so the two cannot drift apart.

BC layouts on a mesh's body marker (2; on testperiodic.msh the two walls 2 and 3) and outer marker (4):
  A  slipwall                 | inflowoutflow     inviscid   fused
  B  slipwall                 | subsonic_inflow   inviscid   staged
  C  adiabaticwall(0.3)       | inflowoutflow     viscous    fused
  D  isothermalwall(0.3, 2.0) | inflowoutflow     viscous    staged
  E  extrapolation            | farfield          inviscid   fused
  F  isothermalwall(0.3, 2.0) | subsonic_inflow   viscous    staged
Viscous layouts come with Sutherland's law ("C") and constant viscosity ("Cc"). On testperiodic.msh the
project's three-marker arrangement (cases.physics("wall")) stays: D and F put the moving adiabatic wall on
marker 2 and the isothermal one on marker 3. The flat plate keeps its decks' four markers: P (plate, the
wall moving at 0.3; Pc constant viscosity), PI (plate_inviscid) and PS (plate_inviscid with subsonic
inflow on marker 5)."""
import numpy as np

import cases
from fvens_amd import FlowBCConfig, FlowPhysicsConfig

G = 1.4
SUBIN = [1.02 / (G * 0.64), 1.01]          # total pressure and temperature of the subsonic inflow
WALL_V, WALL_T = 0.3, 2.0
JUMP = 1.4

BODY = {"A": ("slipwall", []), "B": ("slipwall", []), "C": ("adiabaticwall", [WALL_V]),
        "D": ("isothermalwall", [WALL_V, WALL_T]), "E": ("extrapolation", []),
        "F": ("isothermalwall", [WALL_V, WALL_T])}
OUTER = {"A": ("inflowoutflow", []), "B": ("subsonic_inflow", SUBIN), "C": ("inflowoutflow", []),
         "D": ("inflowoutflow", []), "E": ("farfield", []), "F": ("subsonic_inflow", SUBIN)}
VISCOUS = "CDF"
FUSED_LAYOUTS = ("A", "C", "Cc", "E", "P", "Pc", "PI")
INVISCID_LAYOUTS = ("A", "B", "E")
VISCOUS_LAYOUTS = ("C", "Cc", "D", "Dc", "F", "Fc")
BODY_LAYOUTS = INVISCID_LAYOUTS + VISCOUS_LAYOUTS
PLATE_LAYOUTS = ("P", "Pc", "PI", "PS")


def physics(layout, meshkey):
    """FlowPhysicsConfig of a layout name ("A".."F", "Cc"/"Dc"/"Fc", "P"/"Pc"/"PI"/"PS") on a mesh"""
    const = layout.endswith("c")
    if layout[0] == "P":
        assert meshkey == "plate_small"
        if layout in ("P", "Pc"):
            p = cases.physics("plate")
            p.bcconf[1] = FlowBCConfig("adiabaticwall", 2, [WALL_V])
            p.const_visc = const
        else:
            p = cases.physics("plate_inviscid")
            if layout == "PS":
                p.bcconf[3] = FlowBCConfig("subsonic_inflow", 5, list(SUBIN))
        return p
    L = layout[0]
    body, outer = BODY[L], OUTER[L]
    bcs = [FlowBCConfig(outer[0], 4, list(outer[1]))]
    if meshkey == "testperiodic.msh":
        first = ("adiabaticwall", [WALL_V]) if L in "DF" else body
        bcs += [FlowBCConfig(first[0], 2, list(first[1])), FlowBCConfig(body[0], 3, list(body[1]))]
    else:
        bcs.append(FlowBCConfig(body[0], 2, list(body[1])))
    if L in VISCOUS:
        return FlowPhysicsConfig(gamma=G, Minf=0.8, Tinf=288.15, Reinf=5000.0, Pr=0.72, aoa=1.25 * np.pi / 180,
                                 viscous_sim=True, const_visc=const, bcconf=bcs)
    return FlowPhysicsConfig(gamma=G, Minf=0.8, aoa=1.25 * np.pi / 180, bcconf=bcs)


def calls_pow(layout, rec):
    """the configurations whose residual calls pow (Sutherland, WENO, the subsonic-inflow ghost state):
    compared to 1e-12 of max|r| per variable instead of bitwise"""
    sutherland = layout in ("C", "D", "F", "P")
    subin = layout[0] in "BF" or layout == "PS"
    return sutherland or subin or rec == "WENO"


FIRST_ORDER = [(f, "NONE", "NONE") for f in ("LLF", "ROE", "HLL", "HLLC", "AUSM", "AUSMPLUS", "VANLEER")]
SECOND_ORDER = [("ROE", "LEASTSQUARES", "VANALBADA"), ("HLLC", "LEASTSQUARES", "VANALBADA"),
                ("LLF", "LEASTSQUARES", "VANALBADA"), ("ROE", "GREENGAUSS", "VANALBADA"),
                ("HLLC", "LEASTSQUARES", "NONE"), ("ROE", "LEASTSQUARES", "VENKATAKRISHNAN"),
                ("ROE", "GREENGAUSS", "BARTHJESPERSEN"), ("AUSM", "LEASTSQUARES", "VANALBADA"),
                ("HLL", "GREENGAUSS", "NONE"),
                ("VANLEER", "LEASTSQUARES", "WENO"), ("AUSMPLUS", "LEASTSQUARES", "BARTHJESPERSEN")]
SCHEMES = FIRST_ORDER + SECOND_ORDER
# seeds 3 and 11; on testperiodic.msh (10 faces on marker 4) and the plate (marker 5) seed 3 leaves one of the
# inflow-outflow branches with fewer than 3 faces (and so does 11 on testperiodic.msh), so these two meshes take
# the first seeds that fill the branches and keep the oracle finite in every cell for every scheme
SEEDS = {"testperiodic.msh": (4, 9), "plate_small": (11, 17)}


def seeds(meshkey):
    return SEEDS.get(meshkey, (3, 11))


def numerics(scheme, jac=None):
    flux, grad, rec = scheme
    return cases.numerics(flux, grad, rec, order2=grad != "NONE", jac=jac)


def unlimited(scheme):
    return scheme[1] != "NONE" and scheme[2] == "NONE"


# ---- residual and time steps against the oracle -----------------------------------------------------
# Every (layout, scheme) runs on the three .msh fixtures (2dcylinderhybrid.msh: 336 triangles and 64
# quadrangles; naca0012luo.msh and testperiodic.msh: triangles) and on naca_small (3456 triangles, 576
# quadrangles), except unlimited second-order schemes on naca_small's viscous layouts (unlimited reconstruction
# next to its viscous walls leaves the oracle's residual NaN in a few cells). The plate decks run on plate_small
# (quadrangles only), the only mesh with their four markers. A case costs a few milliseconds on the device.
BODY_MESHES = ("2dcylinderhybrid.msh", "testperiodic.msh", "naca0012luo.msh", "naca_small")


def finite_on(meshkey, layout, scheme):
    return not (meshkey == "naca_small" and unlimited(scheme) and layout in VISCOUS_LAYOUTS + ("P", "Pc"))


def _residual_cases():
    out = [(mk, lay, sch) for mk in BODY_MESHES for lay in BODY_LAYOUTS for sch in SCHEMES if finite_on(mk, lay, sch)]
    return out + [("plate_small", lay, sch) for lay in PLATE_LAYOUTS for sch in SCHEMES]


RESIDUAL_CASES = _residual_cases()

# ---- fused = staged = pipelined ------------------------------------------------------------------------
FUSED_FLUXES = ("ROE", "HLLC", "LLF", "AUSMPLUS")
FUSED_RECS = ("VANALBADA", "NONE", "VENKATAKRISHNAN", "BARTHJESPERSEN")


def _fused_cases():
    out = []
    for lay in FUSED_LAYOUTS:
        visc = lay in ("C", "Cc", "P", "Pc")
        for flux in FUSED_FLUXES:
            for rec in FUSED_RECS:
                if visc and rec not in ("VANALBADA", "NONE"):
                    continue                              # fusedEligible: viscous with MUSCL or unlimited only
                sch = (flux, "LEASTSQUARES", rec)
                out += [(mk, lay, sch) for mk in (("plate_small",) if lay[0] == "P" else BODY_MESHES)
                        if finite_on(mk, lay, sch)]
    return out


FUSED_CASES = _fused_cases()
STAGED_ONLY_CASES = [("2dcylinderhybrid.msh", "B", ("ROE", "LEASTSQUARES", "VANALBADA")),
                     ("naca0012luo.msh", "D", ("HLLC", "LEASTSQUARES", "NONE")),
                     ("testperiodic.msh", "Dc", ("ROE", "LEASTSQUARES", "VANALBADA")),
                     ("2dcylinderhybrid.msh", "F", ("ROE", "LEASTSQUARES", "NONE")),
                     ("plate_small", "PS", ("HLLC", "LEASTSQUARES", "VANALBADA"))]

# ---- Jacobian blocks ------------------------------------------------------------------------------------
JAC_FLUXES = ("LLF", "AUSM", "ROE", "HLL", "HLLC")
JAC_MESHES = ("2dcylinderhybrid.msh", "testperiodic.msh", "naca0012luo.msh")
JAC_CASES = ([(mk, lay, jf) for lay in ("A", "E", "Cc", "Dc", "C", "D") for mk in JAC_MESHES for jf in JAC_FLUXES] +
             [("plate_small", lay, jf) for lay in ("PI", "Pc", "P") for jf in JAC_FLUXES])
JAC_SCHEME = ("ROE", "LEASTSQUARES", "VANALBADA")

# ---- matrix-free operator -------------------------------------------------------------------------------
MATFREE_FUSED_CASES = [(mk, lay, sch) for lay in ("A", "Cc")
                       for mk, sch in (("naca_small", ("ROE", "LEASTSQUARES", "VANALBADA")),
                                       ("2dcylinderhybrid.msh", ("HLLC", "LEASTSQUARES", "NONE")),
                                       ("naca0012luo.msh", ("ROE", "LEASTSQUARES", "VANALBADA")))
                       if not (lay == "Cc" and mk == "naca_small" and unlimited(sch))]
MATFREE_ORACLE_CASES = [(mk, lay, sch) for lay in ("A", "B")
                        for mk, sch in (("2dcylinderhybrid.msh", FIRST_ORDER[1]),
                                        ("naca0012luo.msh", ("ROE", "LEASTSQUARES", "VANALBADA")),
                                        ("naca_small", ("ROE", "LEASTSQUARES", "VANALBADA")))]

# ---- partitioned ----------------------------------------------------------------------------------------
PARTITION_SCHEMES = [("ROE", "LEASTSQUARES", "VANALBADA"), ("HLLC", "LEASTSQUARES", "VENKATAKRISHNAN")]
PARTITION_CASES = [(mk, lay, sch) for mk, lay in (("naca0012luo.msh", "A"), ("naca0012luo.msh", "B"),
                                                  ("plate_small", "P")) for sch in PARTITION_SCHEMES]


def all_cases():
    """every (meshkey, layout, scheme, jac flux or None) a GPU regime test runs, without repeats"""
    seen, out = set(), []
    for mk, lay, sch in RESIDUAL_CASES + FUSED_CASES + STAGED_ONLY_CASES + MATFREE_FUSED_CASES + \
            MATFREE_ORACLE_CASES + PARTITION_CASES:
        if (mk, lay, sch, None) not in seen:
            seen.add((mk, lay, sch, None))
            out.append((mk, lay, sch, None))
    for mk, lay, jf in JAC_CASES:
        out.append((mk, lay, JAC_SCHEME, jf))
    return out


def case_id(c):
    return "-".join(str(x) if not isinstance(x, tuple) else "_".join(x) for x in c if x is not None)


# ---- census: which branches a state reaches on a mesh, from the inputs alone ----------------------------
def census(mesh, p, u):
    """counts of faces per branch of the device code, computed in numpy from the mesh and the cell states:
    per boundary marker the three inflow-outflow branches of the interior state's normal Mach number, and
    over interior faces the supersonic wave-speed and Mach-number branches and faces between cells at rest"""
    g = p.gamma
    nb, nin = mesh.nbface, mesh.naface - mesh.nbface - mesh.nconnface
    rho = u[:, 0]
    vx, vy = u[:, 1] / rho, u[:, 2] / rho
    pr = (g - 1.0) * (u[:, 3] - 0.5 * rho * (vx * vx + vy * vy))
    c = np.sqrt(g * pr / rho)
    fm = mesh.facemetric
    out = {}
    host = mesh.intfac[:nb, 0]
    mni = (vx[host] * fm[:nb, 0] + vy[host] * fm[:nb, 1]) / c[host]
    for tag in np.unique(mesh.btags[:, 0]):
        s = mesh.btags[:, 0] == tag
        out[int(tag)] = {"inflow": int(np.sum(mni[s] <= 0)), "sub_out": int(np.sum((mni[s] > 0) & (mni[s] < 1))),
                         "sup_out": int(np.sum(mni[s] >= 1))}
    L, R = mesh.intfac[nb:nb + nin, 0], mesh.intfac[nb:nb + nin, 1]
    nx, ny = fm[nb:nb + nin, 0], fm[nb:nb + nin, 1]
    vnl, vnr = vx[L] * nx + vy[L] * ny, vx[R] * nx + vy[R] * ny
    sl = np.minimum(vnl - c[L], vnr - c[R])
    sr = np.maximum(vnl + c[L], vnr + c[R])
    rest = (u[L, 1] == 0) & (u[L, 2] == 0) & (u[R, 1] == 0) & (u[R, 2] == 0)
    out["interior"] = {"sl>0": int(np.sum(sl > 0)), "sr<0": int(np.sum(sr < 0)),
                       "Mn>1": int(np.sum((vnl / c[L] > 1) | (vnr / c[R] > 1))),
                       "Mn<-1": int(np.sum((vnl / c[L] < -1) | (vnr / c[R] < -1))), "rest": int(np.sum(rest))}
    return out


def inout_marker(layout):
    """the marker that carries the inflow-outflow BC of a layout, or None"""
    if layout[0] == "P":
        return 5 if layout != "PS" else None
    return 4 if OUTER[layout[0]][0] == "inflowoutflow" else None
