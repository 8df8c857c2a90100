"""GPU parity in every flow regime and boundary type: the residual, Jacobian and matrix-free kernels on
cases.regime_state -- supersonic faces of both signs, sonic lines, cells exactly at rest, jumps that make the
limiters clip -- with BC layouts (regime_cases.py) that run the subsonic-inflow ghost state, all three
inflow-outflow branches and moving adiabatic and isothermal walls on a mesh. The smooth cases.state of the
other mesh-level tests reaches none of these; test_regime_cases_host.py proves, without a GPU, that the oracle
is finite in every cell and every branch is reached for each case run here.

Bars, those of the smooth-state tests:
  * residual and time steps vs the oracle: BITWISE for inviscid and constant-viscosity cases that call no pow;
    Sutherland, WENO and every layout with subsonic inflow (device pow vs glibc pow): |dr| <= 1e-12 max|r| per
    variable, |d dt| <= 1e-12 |dt| (test_gpu_residual.assert_close);
  * fused = staged = pipelined: BITWISE (the same device arithmetic);
  * Jacobian blocks vs the oracle: BITWISE inviscid and constant viscosity, 1e-12 per block entry Sutherland;
  * matrix-free operator: fused BITWISE the three-launch one; 1e-6 of max|y| against the oracle.
A NaN on the device where the oracle is finite is a mismatch."""
import numpy as np
import pytest

import fvens_amd as fa
import _oracle as orc
import cases
import regime_cases as rcs
from test_gpu_residual import assert_close, get_mesh

pytestmark = pytest.mark.gpu

_ref = {}


def state(meshkey, layout, seed):
    m, _ = get_mesh(meshkey)
    return cases.regime_state(m, rcs.physics(layout, meshkey), seed, rcs.JUMP)


def oracle_residual(meshkey, layout, scheme, seed):
    """the oracle's (r, dt) of a case, computed once and shared"""
    key = (meshkey, layout, scheme, seed)
    if key not in _ref:
        m, om = get_mesh(meshkey)
        p = rcs.physics(layout, meshkey)
        r0, dt0 = np.zeros((m.nelem, 4)), np.zeros(m.nelem)
        orc.OracleSpatial(om, p, rcs.numerics(scheme)).compute_residual(state(meshkey, layout, seed), r0, True, dt0)
        assert np.all(np.isfinite(r0)) and np.all(np.isfinite(dt0))
        r0.setflags(write=False)
        dt0.setflags(write=False)
        _ref[key] = (r0, dt0)
    return _ref[key]


def rel_err(r, r0):
    return (np.abs(r - r0).max(axis=0) / (np.abs(r0).max(axis=0) + 1e-300)).max()


RES_GROUPS = sorted({(c[0], c[1]) for c in rcs.RESIDUAL_CASES})


@pytest.mark.parametrize("meshkey,layout", RES_GROUPS, ids=lambda x: str(x))
def test_residual_vs_oracle(meshkey, layout):
    """compute_residual through the C-ABI vs the oracle for every scheme of regime_cases.RESIDUAL_CASES on this
    mesh and layout (the seven first-order fluxes, SECOND_ORDER of test_gpu_residual.py, Van Leer + WENO and
    AUSM+ + Barth-Jespersen), both seeds. Ghost states: abc.cpp:46-81 (inflow-outflow), :145-175 (subsonic
    inflow), :278-287 and :349-366 (moving walls); fluxes: anumericalflux.cpp; limiters:
    limitedlinearreconstruction.cpp.
    Measured on MI355X, the largest relative difference of the pow cases over meshes, schemes and seeds
    (772 comparisons; bar 1e-12): subsonic inflow 6.6e-16 residual / 6.4e-16 time step, Sutherland 6.6e-16 /
    6.4e-16 (Sutherland alone, layouts C, D, P: 1.2e-16 / 6.4e-16), WENO 4.5e-16 / 4.8e-16. Every other case is
    bitwise."""
    m, _ = get_mesh(meshkey)
    p = rcs.physics(layout, meshkey)
    bad = []
    worst = 0.0
    for c in rcs.RESIDUAL_CASES:
        if (c[0], c[1]) != (meshkey, layout):
            continue
        scheme = c[2]
        dev = fa.FlowFV(m, p, rcs.numerics(scheme))
        for seed in rcs.seeds(meshkey):
            r0, dt0 = oracle_residual(meshkey, layout, scheme, seed)
            r, dt = np.zeros((m.nelem, 4)), np.zeros(m.nelem)
            dev.compute_residual(state(meshkey, layout, seed), r, True, dt)
            name = "%s seed %d" % ("_".join(scheme), seed)
            if not (np.all(np.isfinite(r)) and np.all(np.isfinite(dt))):
                bad.append(name + ": device not finite in %d cells" % int((~np.isfinite(r).all(axis=1)).sum()))
            elif rcs.calls_pow(layout, scheme[2]):
                er, et = rel_err(r, r0), (np.abs(dt - dt0) / np.abs(dt0)).max()
                worst = max(worst, er, et)
                print("POW %s %s %s: residual %.3e time step %.3e" % (meshkey, layout, name, er, et))
                try:
                    assert_close(r, r0, dt, dt0)
                except AssertionError as e:
                    bad.append(name + ": " + str(e))
            elif not (np.array_equal(r, r0) and np.array_equal(dt, dt0)):
                bad.append(name + ": not bitwise, residual %.3e in %d cells, time step in %d cells"
                           % (rel_err(r, r0), int((r != r0).any(axis=1).sum()), int((dt != dt0).sum())))
        dev.close()
    print("POWMAX %s %s %.3e" % (meshkey, layout, worst))
    assert not bad, "\n".join(bad)


def _device_residuals(dev, m, u, modes):
    import torch
    perm = dev.permutation()
    du = torch.tensor(u[perm], device="cuda")
    out = []
    for mode in modes:
        dr = torch.full((m.nelem, 4), float("nan"), dtype=torch.float64, device="cuda")
        dt = torch.full((m.nelem,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dev.compute_residual_device(du.data_ptr(), dr.data_ptr(), dt.data_ptr(), True, True,
                                    staged=mode == "staged", pipelined=mode == "pipelined")
        dev.synchronize()
        r, t = np.empty((m.nelem, 4)), np.empty(m.nelem)
        r[perm] = dr.cpu().numpy()
        t[perm] = dt.cpu().numpy()
        out.append((r, t))
    return out


def fused_kernel_launches(dev, m, u):
    """launches of the one-launch residual kernel in one default-path residual (kernel_times)"""
    import torch
    du = torch.tensor(u[dev.permutation()], device="cuda")
    dr = torch.zeros((m.nelem, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev.profile(True)
    dev.compute_residual_device(du.data_ptr(), dr.data_ptr())
    kt = dev.kernel_times()
    dev.profile(False)
    assert kt, "no kernel recorded"
    return sum(cnt for name, (_, cnt) in kt.items() if name.startswith("k_residual_wls"))


FUSED_GROUPS = sorted({(c[1], c[2][0]) for c in rcs.FUSED_CASES})


@pytest.mark.parametrize("layout,flux", FUSED_GROUPS, ids=lambda x: str(x))
def test_fused_equals_staged_equals_pipelined_bitwise(layout, flux):
    """layouts A, C, E and the plate decks: the one-launch residual ran (its kernel is in kernel_times) and is
    bitwise the staged and the pipelined residual, and the oracle where the case calls no pow"""
    for c in rcs.FUSED_CASES:
        if (c[1], c[2][0]) != (layout, flux):
            continue
        meshkey, _, scheme = c
        m, _ = get_mesh(meshkey)
        dev = fa.FlowFV(m, rcs.physics(layout, meshkey), rcs.numerics(scheme))
        for seed in rcs.seeds(meshkey):
            u = state(meshkey, layout, seed)
            assert fused_kernel_launches(dev, m, u) == 1, (meshkey, scheme)
            fused, staged, piped = _device_residuals(dev, m, u, ("fused", "staged", "pipelined"))
            msg = "%s %s seed %d" % (meshkey, "_".join(scheme), seed)
            assert np.all(np.isfinite(fused[0])) and np.all(np.isfinite(fused[1])), msg
            for other in (staged, piped):
                np.testing.assert_array_equal(fused[0], other[0], err_msg=msg)
                np.testing.assert_array_equal(fused[1], other[1], err_msg=msg)
            if not rcs.calls_pow(layout, scheme[2]):
                r0, dt0 = oracle_residual(meshkey, layout, scheme, seed)
                np.testing.assert_array_equal(fused[0], r0, err_msg=msg)
                np.testing.assert_array_equal(fused[1], dt0, err_msg=msg)
        dev.close()


@pytest.mark.parametrize("case", rcs.STAGED_ONLY_CASES, ids=rcs.case_id)
def test_staged_layouts_do_not_take_the_fused_kernel(case):
    """layouts B, D, F (subsonic inflow, isothermal wall): the default path launches no fused kernel, and is
    bitwise the explicitly staged and the pipelined residual"""
    meshkey, layout, scheme = case
    m, _ = get_mesh(meshkey)
    dev = fa.FlowFV(m, rcs.physics(layout, meshkey), rcs.numerics(scheme))
    u = state(meshkey, layout, rcs.seeds(meshkey)[0])
    assert fused_kernel_launches(dev, m, u) == 0
    default, staged, piped = _device_residuals(dev, m, u, ("default", "staged", "pipelined"))
    dev.close()
    assert np.all(np.isfinite(default[0])) and np.all(np.isfinite(default[1]))
    for other in (staged, piped):
        np.testing.assert_array_equal(default[0], other[0])
        np.testing.assert_array_equal(default[1], other[1])


JAC_GROUPS = sorted({(c[0], c[1]) for c in rcs.JAC_CASES})


@pytest.mark.parametrize("meshkey,layout", JAC_GROUPS, ids=lambda x: str(x))
def test_assemble_jacobian_vs_oracle(meshkey, layout):
    """assemble_jacobian vs the oracle's Spatial::assemble_jacobian (aspatial.cpp:242-340) with the BC Jacobians
    of abc.cpp:83-133 (all three inflow-outflow branches), :289-310 and :368-404 (moving walls) and the flux
    Jacobians' supersonic branches: bitwise, Sutherland layouts (C, D, P) to 1e-12 per block entry (measured on
    MI355X: at most 2.5e-16)"""
    m, om = get_mesh(meshkey)
    p = rcs.physics(layout, meshkey)
    bad = []
    for jf in rcs.JAC_FLUXES:
        n = rcs.numerics(rcs.JAC_SCHEME, jac=jf)
        dev = fa.FlowFV(m, p, n)
        ref = orc.OracleSpatial(om, p, n)
        for seed in rcs.seeds(meshkey):
            u = state(meshkey, layout, seed)
            got, exp = dev.assemble_jacobian(u), ref.jacobian(u)
            for a, b, nm in zip(got, exp, ("diag", "lower", "upper")):
                assert np.all(np.isfinite(b))
                if not np.all(np.isfinite(a)):
                    bad.append("%s seed %d %s: device not finite" % (jf, seed, nm))
                elif layout in ("C", "D", "P"):
                    err = (np.abs(a - b).max(axis=0) / (np.abs(b).max(axis=0) + 1e-300)).max()
                    print("POWJAC %s %s %s seed %d %s %.3e" % (meshkey, layout, jf, seed, nm, err))
                    if not err <= 1e-12:
                        bad.append("%s seed %d %s: rel err %.3e" % (jf, seed, nm, err))
                elif not np.array_equal(a, b):
                    bad.append("%s seed %d %s: not bitwise in %d blocks, max |d| %.3e"
                               % (jf, seed, nm, int((a != b).any(axis=(1, 2)).sum()), np.abs(a - b).max()))
        dev.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", rcs.MATFREE_FUSED_CASES, ids=rcs.case_id)
def test_fused_matfree_operator_bitwise(case):
    """layout A and C with constant viscosity: the matrix-free operator fused into one launch of the residual
    kernel against the three-launch operator a one-handle group runs, bitwise on the regime state"""
    import torch
    meshkey, layout, scheme = case
    m, _ = get_mesh(meshkey)
    p, n = rcs.physics(layout, meshkey), rcs.numerics(scheme)
    h1, h2 = fa.FlowFV(m, p, n), fa.FlowFV(m, p, n)
    grp = fa.FlowFVGroup([h2])
    perm = h1.permutation()
    rng = np.random.default_rng(3)
    du = torch.tensor(state(meshkey, layout, rcs.seeds(meshkey)[0])[perm], device="cuda")
    dr = torch.tensor(rng.standard_normal((m.nelem, 4)) * 1e-3, device="cuda")
    dmdt = torch.tensor(rng.random(m.nelem) + 0.5, device="cuda")
    dx = torch.tensor(rng.standard_normal((m.nelem, 4)), device="cuda")
    y1, y2 = torch.zeros_like(dx), torch.zeros_like(dx)
    torch.cuda.synchronize()
    h1.matfree_set_state_device(du.data_ptr(), dr.data_ptr(), dmdt.data_ptr())
    grp.matfree_set_state_device([du.data_ptr()], [dr.data_ptr()], [dmdt.data_ptr()])
    h1.matfree_apply_device(dx.data_ptr(), y1.data_ptr())
    grp.matfree_apply_device([dx.data_ptr()], [y2.data_ptr()])
    h1.synchronize()
    h2.synchronize()
    same, err = torch.equal(y1, y2), float((y1 - y2).abs().max())
    finite, big = bool(torch.isfinite(y1).all()), float(y1.abs().max())
    grp.close()
    h1.close()
    h2.close()
    assert finite and big > 0
    assert same, err


@pytest.mark.parametrize("case", rcs.MATFREE_ORACLE_CASES, ids=rcs.case_id)
def test_matfree_vs_oracle(case):
    """MatrixFreeSpatialJacobian::apply (alinalg.cpp:142-233) on layouts A and B (the first time the
    subsonic-inflow ghost state goes through the operator) against the oracle: the 1e-6 of max|y| of
    test_gpu_jacobian.test_matfree_vs_oracle; x drawn once with a fixed seed. Measured on MI355X: layout A at
    most 8.3e-16, layout B (device pow against glibc pow, divided by eps) at most 1.3e-8; no face flipped a
    branch under the perturbation"""
    meshkey, layout, scheme = case
    m, om = get_mesh(meshkey)
    p, n = rcs.physics(layout, meshkey), rcs.numerics(scheme)
    seed = rcs.seeds(meshkey)[0]
    u = state(meshkey, layout, seed)
    N = m.nelem
    ref = orc.OracleSpatial(om, p, n)
    res, dtm = np.zeros((N, 4)), np.zeros(N)
    ref.compute_residual(u, res, True, dtm)
    mdt = m.area[:N] / (5.0 * dtm)
    x = np.random.default_rng(1).standard_normal((N, 4))
    y0 = ref.matfree(u, res, mdt, 1e-7, x)
    assert np.all(np.isfinite(y0))
    dev = fa.FlowFV(m, p, n)
    dev.matfree_set_state(u, res, mdt)
    y = dev.matfree_apply(x)
    dev.close()
    assert np.all(np.isfinite(y))
    err = np.abs(y - y0).max() / np.abs(y0).max()
    print("MATFREE %s %.3e" % (rcs.case_id(case), err))
    assert err <= 1e-6, err
