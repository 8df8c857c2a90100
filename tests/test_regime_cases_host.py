"""CPU test that keeps the GPU regime tests honest (oracle and numpy only): for every (mesh, layout, scheme,
seed) of regime_cases.py -- the list test_gpu_regimes.py and the regime cases of test_gpu_partition.py run --
  * the oracle's residual, time steps and, where the layout has one, Jacobian are finite in EVERY cell: a
    condition on the case, not a tolerance (a case that fails it gets another mesh or seed, no cell is masked);
  * the branch census, computed in numpy from the mesh and the state alone, shows that the case reaches what
    it is there to reach: at least 3 faces of the inflow-outflow marker in each of Mni <= 0, 0 < Mni < 1 and
    Mni >= 1 (testperiodic.msh, whose marker 4 has 10 faces: the two outflow branches), and at least 10 interior
    faces each with sl > 0, sr < 0, Mn > 1, Mn < -1 and both cells exactly at rest (sl = min(vnL - cL, vnR - cR),
    sr = max(vnL + cL, vnR + cR) on cell states).
The smooth cases.state fails every one of the census assertions (test_census_has_teeth)."""
import numpy as np
import pytest

import _oracle as orc
import cases
import regime_cases as rcs
from test_gpu_residual import get_mesh

ALL = rcs.all_cases()
MESH_LAYOUTS = sorted({(c[0], c[1]) for c in ALL})


def check_census(meshkey, layout, cen):
    bad = [k for k, v in cen["interior"].items() if v < 10]
    tag = rcs.inout_marker(layout)
    if tag is not None:
        need = ("sub_out", "sup_out") if meshkey == "testperiodic.msh" else ("inflow", "sub_out", "sup_out")
        bad += [k for k in need if cen[tag][k] < 3]
    return bad


@pytest.mark.parametrize("meshkey,layout", MESH_LAYOUTS, ids=lambda x: str(x))
def test_branch_census(meshkey, layout):
    m, _ = get_mesh(meshkey)
    p = rcs.physics(layout, meshkey)
    for seed in rcs.seeds(meshkey):
        cen = rcs.census(m, p, cases.regime_state(m, p, seed, rcs.JUMP))
        assert not check_census(meshkey, layout, cen), (seed, cen)


def test_census_has_teeth():
    """on the smooth perturbed free stream every census count is zero: no supersonic face, no cell at rest,
    one inflow-outflow branch per face side of the mesh"""
    for meshkey, layout in MESH_LAYOUTS:
        m, _ = get_mesh(meshkey)
        p = rcs.physics(layout, meshkey)
        cen = rcs.census(m, p, cases.state(m, p, 3))
        assert all(v == 0 for v in cen["interior"].values()), cen
        assert len(check_census(meshkey, layout, cen)) >= 5


def test_regime_state_is_deterministic_and_at_rest_exactly():
    m, _ = get_mesh("2dcylinderhybrid.msh")
    p = rcs.physics("A", "2dcylinderhybrid.msh")
    u = cases.regime_state(m, p, 3)
    np.testing.assert_array_equal(u, cases.regime_state(m.rc[:m.nelem], p, 3))
    assert not np.array_equal(u, cases.regime_state(m, p, 11))
    rest = (u[:, 1] == 0) & (u[:, 2] == 0)
    assert rest.sum() >= 20 and not np.signbit(u[rest, 1:3]).any()
    pr = 0.4 * (u[:, 3] - 0.5 * (u[:, 1] ** 2 + u[:, 2] ** 2) / u[:, 0])
    mach = np.hypot(u[:, 1], u[:, 2]) / u[:, 0] / np.sqrt(1.4 * pr / u[:, 0])
    assert mach.max() > 1.9 and np.all(pr > 0) and np.all(u[:, 0] > 0)


@pytest.mark.parametrize("meshkey,layout", MESH_LAYOUTS, ids=lambda x: str(x))
def test_oracle_finite(meshkey, layout):
    m, om = get_mesh(meshkey)
    p = rcs.physics(layout, meshkey)
    N = m.nelem
    bad = []
    for c in ALL:
        if (c[0], c[1]) != (meshkey, layout):
            continue
        ref = orc.OracleSpatial(om, p, rcs.numerics(c[2], jac=c[3]))
        for seed in rcs.seeds(meshkey):
            u = cases.regime_state(m, p, seed, rcs.JUMP)
            if c[3] is None:
                r, dt = np.zeros((N, 4)), np.zeros(N)
                ref.compute_residual(u, r, True, dt)
                nbad = int((~np.isfinite(r).all(axis=1) | ~np.isfinite(dt)).sum())
                if nbad or not np.all(dt > 0):
                    bad.append((rcs.case_id(c), seed, nbad))
            else:
                nbad = sum(int((~np.isfinite(a)).sum()) for a in ref.jacobian(u))
                if nbad:
                    bad.append((rcs.case_id(c), seed, nbad))
    assert not bad, bad


@pytest.mark.parametrize("case", rcs.MATFREE_ORACLE_CASES, ids=rcs.case_id)
def test_oracle_matfree_finite(case):
    """the oracle's matrix-free product of the GPU test's x (rng seed 1) is finite in every cell"""
    meshkey, layout, scheme = case
    m, om = get_mesh(meshkey)
    p = rcs.physics(layout, meshkey)
    u = cases.regime_state(m, p, rcs.seeds(meshkey)[0], rcs.JUMP)
    ref = orc.OracleSpatial(om, p, rcs.numerics(scheme))
    res, dtm = np.zeros((m.nelem, 4)), np.zeros(m.nelem)
    ref.compute_residual(u, res, True, dtm)
    x = np.random.default_rng(1).standard_normal((m.nelem, 4))
    y0 = ref.matfree(u, res, m.area[:m.nelem] / (5.0 * dtm), 1e-7, x)
    assert np.all(np.isfinite(y0)) and np.abs(y0).max() > 0
