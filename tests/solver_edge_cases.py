"""Size edges of the solver stack: the meshes, systems and case lists of tests/test_solver_edge_host.py (CPU) and
tests/test_gpu_solver_edge.py (device). The host file proves every listed case (finite system, host forms agreeing,
teeth); the device file runs exactly these lists.

Meshes, all UMesh.flat_plate(nx, ny) with the plate_inviscid physics:
  P11 (1,1)  one cell, no interior face (lower / upper empty, their pointers null), Krylov dimension 4, one line of
             one cell, one colour, every preconditioner exact
  P21 (2,1)  one interior face, two colours
  P13 (1,3)  one line of three cells; split three ways every rank owns one cell and has no face of its own
  P32 (3,2)  six cells, seven interior faces; split by column three ranks of two cells
  Cn  (1,n)  n = 2, 15, 16, 17, 18, 20, 22, 257: one wall-normal column. Its cells' coupling ratios are the column's
             stretching (1 at both ends), all below the default line threshold 4, where every cell is a line of its
             own; at LINE_THRESHOLD = 1 (every cell qualifies) the column is one line, cut at 256 cells. A twisted
             line of n cells runs a top half of (n-1)/2 + 1 and a bottom half of n - (n-1)/2 cells: 8|9, 9|9, 9|10,
             10|11, 11|12 for n = 16 .. 22, so (half - 1) % 4, k_line_solve_rows' remainder, takes 3, 0, 1, 2.
Numerics: Roe + least squares + Van Albada on every mesh; the oracle's residual, time steps and Jacobian are finite in
every cell of each (test_system_is_finite), so the first-order fallback is not needed.

Cases the host test removed, and why:
  * stand-alone GMRES beyond STANDALONE_KMAX: with s Jacobi sweeps A M^-1 has few distinct eigenvalues on these meshes
    and GMRES ends early, so one more step, or the other sweep count, no longer moves x by 1000 bars. P11 has no
    k-th-iterate case at all (every preconditioner is exact on one cell); it has its own one-iteration cases.
  * the line solve and ILU(0) with k >= 2 on P21 and P13 on one handle (EXACT): one line covers the mesh, and ILU(0)
    of a chain of cells drops nothing, so M = A and GMRES stops after one step. (60, 1) stays: the iterate is
    A^-1 b. Their other sweep counts and colour orders are the same operator and are not told apart.
  * Gauss-Seidel with three sweeps at (60, 2) on P21 (REMOVED_STEP): four sweeps are within 560 bars.
On the three ranks of P13 every rank owns one cell and has no face of its own, so Gauss-Seidel, ILU(0) and the line
solve are block Jacobi there (test_p13_ranks_are_block_jacobi records it); they are told apart from one domain's
forms, not from each other.
Measured on the CPU (tests/test_solver_edge_host.py prints them as FLOOR lines), the largest difference between host
forms over each family's cases; 1, 3 and 8 BLAS threads give the same figures (the matrices are too small for the
thread count to change a summation order), and the constants are four times them where that is above the project's:
  stand-alone, of max |x|                       7.4e-15   -> gh.FLOOR["fast"] = 3.2e-14  (smallest step 3.3e-8)
  step, Jacobi / Gauss-Seidel / ILU(0), fp64    5.1e-15 / 4.6e-15 / 3.5e-15, fp32 8.9e-15 / 3.5e-15 / 4.3e-15,
        3 ranks 3.7e-15 / 3.1e-15 / 3.9e-15     -> gh.FLOOR["jacobian"] = 2e-14  (smallest step 2.5e-2)
  step, lines, of max |du| per variable         5.1e-14 on one handle, 3.3e-14 on 3 ranks -> 2.1e-13: the host's line
        solve is scipy's sparse LU of a matrix whose entries span the column's 1e-4 wall spacing (smallest step 0.9)
  line solve against the dense solve, max |z|   9.1e-16   -> gh.FLOOR["jacobian"] = 2e-14
"""
import functools
from types import SimpleNamespace

import numpy as np

import fvens_amd as fa
import _oracle as orc
import cases
import gmres_host as gh

P_MESHES = {"P11": (1, 1), "P21": (2, 1), "P13": (1, 3), "P32": (3, 2)}
C_LENGTHS = (2, 15, 16, 17, 18, 20, 22, 257)
PHYSICS = "plate_inviscid"
NUMERICS = ("ROE", "LEASTSQUARES", "VANALBADA")
LINE_THRESHOLD = 1.0
LINE_MAX_CELLS = 256
# explicit partitions of the groups: cell j*nx + i
PARTS = {"P13": np.array([0, 1, 2], np.int32), "P32": np.array([0, 1, 2, 0, 1, 2], np.int32)}

# ---- measured on the host, never on the device ----------------------------------------------------------------------
# largest disagreement between host forms per family (max over 1, 3 and 8 BLAS threads, times four); where it is under
# gh.FLOOR["jacobian"] (fast: gh.FLOOR["fast"]) that constant is the floor
FLOORS = {"standalone": gh.FLOOR["fast"], "step": gh.FLOOR["jacobian"], "step_lines": 2.1e-13,
          "line_dense": gh.FLOOR["jacobian"]}
BAR = {k: gh.BAR_FACTOR * v for k, v in FLOORS.items()}


def step_family(kind):
    return "step_lines" if kind == "lines" else "step"

# ---- case lists -----------------------------------------------------------------------------------------------------
# stand-alone GMRES, (mesh, restart, k, sweeps): rtol 0, maxit k
# k = 1 .. the largest k at which one more step and the other sweep count both move x by 1000 bars (later steps are
# at rounding: with s sweeps A M^-1 = I - (-E)^s has few distinct eigenvalues on these meshes, and GMRES ends early)
STANDALONE_KMAX = {("P21", 1): 7, ("P21", 2): 4, ("P13", 1): 7, ("P13", 2): 4, ("P32", 1): 10, ("P32", 2): 6}
STANDALONE_CASES = ([(name, 60, k, s) for (name, s), kmax in STANDALONE_KMAX.items() for k in range(1, kmax + 1)]
                    + [("P21", 2, 5, 1), ("P21", 2, 5, 2)])        # restart below the dimension
EXHAUST_CASES = [(name, s) for name in ("P11", "P21", "P13", "P32") for s in (1, 2)]
EXHAUST_RTOL, EXHAUST_RESTART = 1e-10, 60
# one backward-Euler step, (restart, k); kinds gh.PREC_KINDS, prec_single for all but lines
STEP_RK = [(60, 1), (60, 2), (1, 2)]
STEP_MESHES = ("P21", "P13", "P32")
# M = A exactly: one line covers P21 and P13, and ILU(0) of a chain of cells has no fill to drop. Only k = 1, and no
# other sweep count to tell apart
EXACT = {"lines": ("P21", "P13"), "ilu": ("P21", "P13")}
# three Gauss-Seidel sweeps on two cells all but solve the system: four sweeps move the second iterate by 560 bars
REMOVED_STEP = {("P21", "gs", 3, 60, 2)}


def exact(name, kind):
    return name in EXACT.get(kind, ())


def step_cases():
    out = []
    for name in STEP_MESHES:
        for kind, sweeps in gh.PREC_KINDS:
            for restart, k in STEP_RK:
                if (exact(name, kind) and k > 1) or (name, kind, sweeps, restart, k) in REMOVED_STEP:
                    continue
                for single in ((False,) if kind == "lines" else (False, True)):
                    out.append((name, kind, sweeps, restart, k, single))
    return out


def group_step_cases():
    return [(name, kind, sweeps, 60, 2) for name in PARTS for kind, sweeps in gh.PREC_GROUP_KINDS]


DRIVER_STEPS = 3
DRIVER_CFL = 0.4
# (driver, order, mode): forward Euler, TVD-RK and SSP-RK of orders 1-3, SSP-RK in CFL and fixed-dt mode
DRIVER_CASES = ([("fe", 1, "cfl")] + [("tvdrk", o, "cfl") for o in (1, 2, 3)]
                + [("ssprk", o, mode) for o in (1, 2, 3) for mode in ("cfl", "dt")])
DIVERGED = {"fe": "Steady forward Euler diverged - residual is Nan or inf!", "tvdrk": "dtmin is Nan or inf",
            "ssprk": "SSP-RK diverged - dtmin is Nan or inf!"}
SECOND_TRIP_LANES = 512 * 256          # RED_CELL_BLOCKS x 256


# ---- meshes and systems ---------------------------------------------------------------------------------------------

def mesh_shape(name):
    return P_MESHES[name] if name in P_MESHES else (1, int(name[1:]))


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(UMesh, OracleMesh) of P11 .. P32 or Cn"""
    m = fa.UMesh.flat_plate(*mesh_shape(name))
    return m, orc.OracleMesh.from_raw(m.raw())


def physics():
    return cases.physics(PHYSICS)


def numerics():
    return cases.numerics(*NUMERICS)


@functools.lru_cache(maxsize=None)
def step_system(name):
    """one backward-Euler step's system (gh._step_system_on: state seed 8, CFL gh.STEP_CFL) on a P or C mesh"""
    m, om = mesh(name)
    return gh._step_system_on(m, om, physics(), numerics())


@functools.lru_cache(maxsize=None)
def fast_system(name):
    """the stand-alone solver's system: gh.random_blocks("fast", ...) on the mesh, x standard normal"""
    m, _ = mesh(name)
    D, lo, up, b = gh.random_blocks("fast", m.nelem, m.naface - m.nbface)
    x = np.random.default_rng(21).standard_normal((m.nelem, 4))
    return SimpleNamespace(m=m, D=D, lo=lo, up=up, b=b, x=x, A=gh.block_matrix(m, D, lo, up), Dinv=gh.block_diag_inverse(D))


@functools.lru_cache(maxsize=None)
def line_blocks(name):
    """the blocks of test_line_solve_inverts_line_blocks (D = N(0,1) + 16 I, off-diagonal 0.5 N(0,1)) and v"""
    m, _ = mesh(name)
    N, Fi = m.nelem, m.naface - m.nbface
    rng = np.random.default_rng(3)
    D = rng.standard_normal((N, 4, 4)) + 16.0 * np.eye(4)[None]
    lo, up = 0.5 * rng.standard_normal((Fi, 4, 4)), 0.5 * rng.standard_normal((Fi, 4, 4))
    return SimpleNamespace(m=m, D=D, lo=lo, up=up, v=rng.standard_normal((N, 4)))


def expected_line_lengths(name):
    """the line lengths of a C mesh at LINE_THRESHOLD, longest first"""
    n = mesh_shape(name)[1]
    return [LINE_MAX_CELLS] * (n // LINE_MAX_CELLS) + ([n % LINE_MAX_CELLS] if n % LINE_MAX_CELLS else [])


def line_matrix(s, perm, lines):
    """M of the line solve, dense, in the mesh's cell order: the diagonal blocks and the blocks of consecutive line
    cells, assembled as test_line_solve_inverts_line_blocks does (perm: internal -> mesh cell; lines in internal
    cells, faces fi << 1 | the previous cell is the face's R)"""
    N = s.m.nelem
    M = np.zeros((N, 4, N, 4))
    for c in range(N):
        M[c, :, c, :] = s.D[c]
    for cells, faces in lines:
        for k in range(1, len(cells)):
            c, pv, fi, side = perm[cells[k]], perm[cells[k - 1]], faces[k] >> 1, faces[k] & 1
            a_cp, a_pc = (s.up[fi], s.lo[fi]) if side else (s.lo[fi], s.up[fi])
            M[c, :, pv, :] = a_cp
            M[pv, :, c, :] = a_pc
    return M.reshape(4 * N, 4 * N)


def block_thomas(M, v, T=np.float64):
    """one-ended block Thomas on a block-tridiagonal dense M (4x4 blocks, in order), arithmetic in T"""
    n = v.size // 4
    B = M.astype(T).reshape(n, 4, n, 4)
    g = np.zeros((n, 4), T)
    W = np.zeros((n, 4, 4), T)
    rhs = v.astype(T).reshape(n, 4)

    def solve(a, b):
        return np.linalg.solve(a.astype(np.float64), b.astype(np.float64)).astype(T) if T is np.float64 else _gauss(a, b)
    piv = B[0, :, 0, :]
    g[0] = solve(piv, rhs[0])
    for k in range(1, n):
        W[k - 1] = solve(piv, B[k - 1, :, k, :])
        piv = B[k, :, k, :] - B[k, :, k - 1, :] @ W[k - 1]
        g[k] = solve(piv, rhs[k] - B[k, :, k - 1, :] @ g[k - 1])
    z = np.zeros((n, 4), T)
    z[n - 1] = g[n - 1]
    for k in range(n - 2, -1, -1):
        z[k] = g[k] - W[k] @ z[k + 1]
    return z.reshape(-1)


def _gauss(a, b):
    """Gaussian elimination with partial pivoting in the dtype of a (np.longdouble has no LAPACK)"""
    a = a.copy()
    b = b.copy().reshape(a.shape[0], -1)
    n = a.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]] = a[[p, k]]
            b[[k, p]] = b[[p, k]]
        for i in range(k + 1, n):
            f = a[i, k] / a[k, k]
            a[i, k:] -= f * a[k, k:]
            b[i] -= f * b[k]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - a[k, k + 1:] @ x[k + 1:]) / a[k, k]
    return x.reshape(-1) if x.shape[1] == 1 else x


def long_product(s, x):
    """(A x, |A| |x|) of the face blocks in np.longdouble, rows in the mesh's cell order"""
    m = s.m
    W = np.longdouble
    L, R = m.intfac[m.nbface:, 0].astype(np.int64), m.intfac[m.nbface:, 1].astype(np.int64)
    xl = x.astype(W)
    y = np.einsum("cij,cj->ci", s.D.astype(W), xl)
    a = np.einsum("cij,cj->ci", np.abs(s.D).astype(W), np.abs(xl))
    np.add.at(y, R, np.einsum("fij,fj->fi", s.lo.astype(W), xl[L]))
    np.add.at(a, R, np.einsum("fij,fj->fi", np.abs(s.lo).astype(W), np.abs(xl[L])))
    np.add.at(y, L, np.einsum("fij,fj->fi", s.up.astype(W), xl[R]))
    np.add.at(a, L, np.einsum("fij,fj->fi", np.abs(s.up).astype(W), np.abs(xl[R])))
    return y, a


def rank_of(colour, lines, glob):
    return SimpleNamespace(glob=np.asarray(glob), colour=np.asarray(colour), lines=lines)


# ---- the explicit drivers on the host -------------------------------------------------------------------------------

def driver_state(name):
    m, _ = mesh(name)
    return cases.state(m, physics(), 5)


@functools.lru_cache(maxsize=None)
def fixed_dt(name):
    """the fixed step of SSP-RK's dt mode: DRIVER_CFL times the first minimum time step"""
    import ssprk_host as sh
    _, om = mesh(name)
    return DRIVER_CFL * float(sh.oracle_residual(om, physics(), numerics())(driver_state(name))[1].min())


@functools.lru_cache(maxsize=None)
def host_driver(name, driver, order, mode):
    """the host loop of one driver case: namespace(u, steps, time, rec)"""
    import ssprk_host as sh
    from test_gpu_tvdrk import host_tvdrk
    m, om = mesh(name)
    p, n, u0 = physics(), numerics(), driver_state(name)
    if driver == "fe":
        u = u0.copy()
        steps, ratio = orc.OracleSpatial(om, p, n).forward_euler(u, DRIVER_CFL, 0.0, DRIVER_STEPS)
        return SimpleNamespace(u=u, steps=steps, time=None, rec=None, ratio=ratio)
    if driver == "tvdrk":
        u, steps, t = host_tvdrk(m, om, p, n, u0, order, DRIVER_CFL, 1e9, DRIVER_STEPS)
        return SimpleNamespace(u=u, steps=steps, time=t, rec=None)
    kw = dict(cfl=DRIVER_CFL) if mode == "cfl" else dict(dt=fixed_dt(name))
    u, st, rec = sh.ssprk(sh.oracle_residual(om, p, n), m.area[:m.nelem], u0, order, 1e9, DRIVER_STEPS, **kw)
    return SimpleNamespace(u=u, steps=st["steps"], time=st["time"], rec=rec, stats=st)
