"""Surface functionals on the device: FlowFV_base::computeSurfaceData
(flow_spatial.cpp:130-310) through fvhip_surface_data_device, against the oracle's restatement on the
same state and gradients.

Bars: CL and CDp bitwise (same operations in the same face order; the wind vector and free-stream
pressure are formed on the host as the reference does); CDsf to 1e-12 relative (Sutherland's
T^1.5 is the device pow, which may differ from the host's in the last bit); per-face Cp bitwise
against a numpy restatement of getPressureFromConserved, face centres equal to the mesh's gr.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import fvens_amd as fa
import _oracle as orc
import cases
import functionals_host as fh
from test_gpu_residual import get_mesh

pytestmark = pytest.mark.gpu


def _run(kind, seed):
    import torch
    m, om = get_mesh("naca_small")
    p = cases.physics(kind)
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u = cases.state(m, p, seed)
    dev = fa.FlowFV(m, p, n)
    perm = dev.permutation()
    dU = torch.tensor(np.ascontiguousarray(u[perm]), device="cuda")
    (cl, cdp, cdf), faces = dev.surface_data_device(dU.data_ptr(), 2)
    ref = orc.OracleSpatial(om, p, n)
    rcl, rcdp, rcdf = ref.surface(u, ref.getGradients(u), 2)
    dev.close()
    return m, p, u, (cl, cdp, cdf), faces, (rcl, rcdp, rcdf)


@pytest.mark.parametrize("kind,seed", [("naca", 3), ("visc", 5)])
def test_surface_functionals_match_oracle(kind, seed):
    m, p, u, (cl, cdp, cdf), faces, (rcl, rcdp, rcdf) = _run(kind, seed)
    assert cl == rcl and cdp == rcdp, (cl, rcl, cdp, rcdp)
    assert abs(cdf - rcdf) <= 1e-12 * abs(rcdf), (cdf, rcdf)
    if kind == "visc":
        assert rcdf != 0.0
    # per face, reference boundary-face order: centre and Cp
    nb = m.nbface
    wall = np.nonzero(np.asarray(m.btags).reshape(nb, -1)[:, 0] == 2)[0]
    assert faces.shape == (len(wall), 4)
    L = m.intfac[wall, 0]
    uc = u[L]
    pr = (p.gamma - 1.0) * (uc[:, 3] - (0.5 * (uc[:, 1] * uc[:, 1] + uc[:, 2] * uc[:, 2])) / uc[:, 0])
    pinf = 1.0 / (p.gamma * p.Minf * p.Minf)
    assert np.array_equal(faces[:, 2], (pr - pinf) * 2.0)
    assert np.array_equal(faces[:, :2], np.asarray(m.gr).reshape(-1, 2)[wall])


# ---- edges of the surface functionals: launch shapes, markers, physics, gradient schemes, handle state ----------------
#
# Bars ("Output functionals"): CL and CDp bitwise the oracle's, CDsf 1e-12 of it; all three within
# 1e-12 Sigma|Cp_i| len_i / Sigma len_i of the long-double restatement (tests/functionals_host.py, pinned against the
# oracle on the CPU by tests/test_functionals_host.py); face centres and Cp bitwise numpy; Cf per face within
# 1e-12 max|Cf| of the restatement, and exactly 0.0 wherever the viscosity or the gradients are zero.

OGRID_FACES = (8, 64, 254, 256, 258, 514)          # wall faces: under one wave, one wave, round one block, two blocks
VISCOUS = ("visc", "plate")


def _mesh(key):
    """get_mesh's keys, and ogridN = UMesh.naca_ogrid(N, 2, 2): N faces on each of markers 2 and 4, 6 N cells"""
    if key.startswith("ogrid"):
        if key not in _ogrids:
            m = fa.UMesh.naca_ogrid(int(key[5:]), 2, 2)
            _ogrids[key] = (m, orc.OracleMesh.from_raw(m.raw()))
        return _ogrids[key]
    return get_mesh(key)


_ogrids = {}


def _markers(m):
    return sorted(set(int(t) for t in np.asarray(m.btags).reshape(m.nbface, -1)[:, 0]))


def _physics(phys):
    return cases.physics("visc", aoa_deg=3.0) if phys == "visc_aoa3" else cases.physics(phys.split("_")[0])


def _upload(u, perm):
    import torch
    d = torch.tensor(np.ascontiguousarray(u[perm]), device="cuda")
    torch.cuda.synchronize()         # torch's stream against the library's own
    return d


@functools.lru_cache(maxsize=None)
def _case(meshkey, phys, grad, seed):
    """one handle per (mesh, physics, gradient scheme): the device result for every marker of the mesh in ascending
    order, the oracle's functionals and the long-double rows on the oracle's gradients; computed once"""
    m, om = _mesh(meshkey)
    p = _physics(phys)
    n = cases.numerics("ROE", grad, "VANALBADA")
    u = cases.state(m, p, seed)
    ref = orc.OracleSpatial(om, p, n)
    grads = ref.getGradients(u)
    dev = fa.FlowFV(m, p, n)
    dU = _upload(u, dev.permutation())
    out = {}
    for marker in _markers(m):
        funcs, faces = dev.surface_data_device(dU.data_ptr(), marker)
        rows, prods = fh.surface_rows(m, p, u, grads, marker)
        out[marker] = SimpleNamespace(funcs=funcs, faces=faces.copy(), oracle=ref.surface(u, grads, marker),
                                      rows=rows, prods=prods)
    dev.close()
    return SimpleNamespace(m=m, p=p, u=u, grads=grads, kind=phys.split("_")[0], grad=grad, markers=out)


def _check(c, marker):
    """every per-case assertion of one marker; prints the measured margins before it asserts"""
    m, p, u = c.m, c.p, c.u
    r = c.markers[marker]
    cl, cdp, cdf = r.funcs
    rcl, rcdp, rcdf = (float(x) for x in r.oracle)
    faces, rows, prods = r.faces, r.rows, r.prods
    wall = fh.marker_faces(m, marker)
    viscous = c.kind in VISCOUS and c.grad != "NONE"
    tot = fh.fsum(prods[:, 3])
    scale = float(fh.fsum(np.abs(rows[:, 2]) * prods[:, 3]) / tot)
    mine = [float(x) for x in fh.surface_functionals(prods)]
    cfmax = float(np.abs(rows[:, 3]).max())
    cferr = float(np.abs(faces[:, 3].astype(np.longdouble) - rows[:, 3]).max())
    print("surface %d faces marker %d: functionals - long double %s of the Cp scale; CDsf - oracle %.3g relative; "
          "Cf - long double %.3g of max|Cf| = %.3g"
          % (len(wall), marker, " ".join("%.3g" % (abs(a - b) / scale) for a, b in zip((cl, cdp, cdf), mine)),
             abs(cdf - rcdf) / abs(rcdf) if rcdf != 0 else 0.0, cferr / cfmax if cfmax > 0 else 0.0, cfmax))
    assert faces.shape == (len(wall), 4) and len(wall) > 0
    assert not np.isnan(faces).any() and not np.isnan([cl, cdp, cdf]).any()
    assert cl == rcl and cdp == rcdp, (cl, rcl, cdp, rcdp)
    assert abs(cdf - rcdf) <= 1e-12 * abs(rcdf), (cdf, rcdf)
    for name, a, b in zip(("CL", "CDp", "CDsf"), (cl, cdp, cdf), mine):
        assert abs(a - b) <= 1e-12 * scale, (name, a, b, scale)
    assert np.array_equal(faces[:, :2], np.asarray(m.gr).reshape(-1, 2)[wall])
    uc = u[m.intfac[wall, 0]]
    pr = (p.gamma - 1.0) * (uc[:, 3] - (0.5 * (uc[:, 1] * uc[:, 1] + uc[:, 2] * uc[:, 2])) / uc[:, 0])
    pinf = 1.0 / (p.gamma * p.Minf * p.Minf)
    assert np.array_equal(faces[:, 2], (pr - pinf) * 2.0)
    if not viscous:
        # Re_inf = inf: muhat is exactly 0; no gradients: the stress is exactly 0
        assert np.all(faces[:, 3] == 0.0) and cdf == 0.0 and rcdf == 0.0 and cfmax == 0.0
        return
    tol = 1e-12 * cfmax
    assert cfmax > 0
    assert cferr <= tol, (cferr, cfmax)
    # teeth: on this state the two index mistakes the kernel could make move Cf by more than the tolerance. The
    # gradient block read as [dim][var] is the restatement on the re-read blocks; the tangent negated gives -Cf
    # exactly, 2 max|Cf| away. (Transposing gradu itself is no mistake: the stress is gradu + gradu^T.)
    reread = np.ascontiguousarray(c.grads.reshape(-1, 2, 4).transpose(0, 2, 1))
    assert float(np.abs(fh.surface_rows(m, p, u, reread, marker)[0][:, 3] - rows[:, 3]).max()) > tol
    assert float(np.abs(-rows[:, 3] - rows[:, 3]).max()) > tol


OGRID_PHYSICS = dict(zip(OGRID_FACES, ("visc_aoa3", "naca", "visc_aoa0", "visc_aoa3", "naca", "visc_aoa3")))


@pytest.mark.parametrize("marker", [2, 4], ids=["wall2", "farfield4"])
@pytest.mark.parametrize("ntheta", OGRID_FACES, ids=["faces%d-%s" % (k, OGRID_PHYSICS[k]) for k in OGRID_FACES])
def test_surface_face_counts(ntheta, marker):
    """launch shapes of k_surface_faces on O-grids with ntheta faces per marker, the physics alternating"""
    c = _case("ogrid%d" % ntheta, OGRID_PHYSICS[ntheta], "LEASTSQUARES", 11 + ntheta)
    assert _markers(c.m) == [2, 4] and len(fh.marker_faces(c.m, marker)) == ntheta
    _check(c, marker)


@pytest.mark.parametrize("marker", [2, 3, 4, 5], ids=["plate-adiabaticwall2", "plate-slipwall3", "plate-farfield4", "plate-inflowoutflow5"])
def test_surface_plate_markers(marker):
    c = _case("plate_small", "plate", "LEASTSQUARES", 7)
    assert _markers(c.m) == [2, 3, 4, 5]
    _check(c, marker)


@pytest.mark.parametrize("meshkey,phys", [("2dcylinderhybrid.msh", "cyl"), ("NACA0012_lam_hybrid_1.msh", "visc_aoa0")],
                         ids=["2dcylinderhybrid-cyl-allmarkers", "NACA0012_lam_hybrid_1-visc_aoa0-allmarkers"])
def test_surface_gmsh_markers(meshkey, phys):
    """the hybrid (triangle + quadrangle) Gmsh fixtures, every marker the file holds"""
    c = _case(meshkey, phys, "LEASTSQUARES", 13)
    assert len(c.markers) >= 2 and len(np.unique(c.m.nnode)) == 2
    for marker in c.markers:
        _check(c, marker)


@pytest.mark.parametrize("grad", ["LEASTSQUARES", "GREENGAUSS", "NONE"])
@pytest.mark.parametrize("phys", ["visc_aoa0", "visc_aoa3", "naca"])
def test_surface_gradient_schemes(phys, grad):
    """naca_small: every gradient scheme conservedGradients dispatches on, viscous at two angles and inviscid"""
    c = _case("naca_small", phys, grad, 5)
    for marker in (2, 4):
        _check(c, marker)
    if grad == "NONE":
        assert all(np.all(c.markers[k].faces[:, 3] == 0.0) and c.markers[k].funcs[2] == 0.0 for k in (2, 4))


def _fresh(m, p, n, u, marker):
    dev = fa.FlowFV(m, p, n)
    dU = _upload(u, dev.permutation())
    out = dev.surface_data_device(dU.data_ptr(), marker)
    dev.close()
    return out


def _same(a, b):
    return np.array_equal(np.asarray(a[0]), np.asarray(b[0]), equal_nan=True) and np.array_equal(a[1], b[1])


def test_surface_marker_without_faces():
    """a marker the mesh does not have: 0/0 as the reference (flow_spatial.cpp:307), zero rows, no error, and the
    handle goes on working"""
    m, _ = get_mesh("naca_small")
    p, n = cases.physics("visc", aoa_deg=3.0), cases.numerics()
    u = cases.state(m, p, 5)
    assert 7 not in _markers(m)
    dev = fa.FlowFV(m, p, n)
    dU = _upload(u, dev.permutation())
    before = dev.surface_data_device(dU.data_ptr(), 2)
    for _ in range(2):                     # the second call takes the cached (empty) face list
        funcs, faces = dev.surface_data_device(dU.data_ptr(), 7)
        assert faces.shape == (0, 4) and all(np.isnan(x) for x in funcs), (funcs, faces.shape)
    after = dev.surface_data_device(dU.data_ptr(), 2)
    dev.close()
    assert _same(before, after) and not np.isnan(after[0]).any()
    assert _same(after, _fresh(m, p, n, u, 2))


def test_surface_marker_cache():
    """markers 2, 4, 2 on one handle, the third call on another state: each bitwise a fresh handle's"""
    m, _ = get_mesh("naca_small")
    p, n = cases.physics("visc", aoa_deg=3.0), cases.numerics()
    ua, ub = cases.state(m, p, 5), cases.state(m, p, 6)
    dev = fa.FlowFV(m, p, n)
    perm = dev.permutation()
    dA, dB = _upload(ua, perm), _upload(ub, perm)
    got = [dev.surface_data_device(dA.data_ptr(), 2), dev.surface_data_device(dA.data_ptr(), 4),
           dev.surface_data_device(dB.data_ptr(), 2)]
    got = [(f, faces.copy()) for f, faces in got]
    dev.close()
    want = [_fresh(m, p, n, ua, 2), _fresh(m, p, n, ua, 4), _fresh(m, p, n, ub, 2)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (k, g[0], w[0])
    assert not _same(got[0], got[2])       # the third call saw the other state


@pytest.mark.parametrize("staged", [False, True], ids=["fused", "staged"])
def test_surface_call_leaves_the_residual_alone(staged):
    """conservedGradients overwrites d_up, d_ubc, d_ug and d_grad: a residual after the functionals (surface and
    entropy) is bitwise the one before"""
    import torch
    m, _ = get_mesh("naca_small")
    p, n = cases.physics("visc", aoa_deg=3.0), cases.numerics()
    u, other = cases.state(m, p, 5), cases.state(m, p, 6)
    dev = fa.FlowFV(m, p, n)
    perm = dev.permutation()
    dU, dO = _upload(u, perm), _upload(other, perm)

    def residual():
        dr = torch.zeros((m.nelem, 4), dtype=torch.float64, device="cuda")
        dt = torch.zeros(m.nelem, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dev.compute_residual_device(dU.data_ptr(), dr.data_ptr(), dt.data_ptr(), True, True, staged=staged)
        dev.synchronize()
        return dr.cpu().numpy(), dt.cpu().numpy()
    r0, t0 = residual()
    dev.surface_data_device(dO.data_ptr(), 2)          # another state: the scratch arrays now hold its gradients
    dev.entropy_error_device(dO.data_ptr())
    r1, t1 = residual()
    dev.close()
    assert np.abs(r0).max() > 0 and np.all(t0 > 0)
    assert np.array_equal(r0, r1) and np.array_equal(t0, t1)


def test_partitioned_handle_without_communicator_refuses():
    """no group-level surface call exists: a rank's handle without its communicator must refuse, not return its
    local sums over its local length"""
    import torch
    m, _ = get_mesh("naca_small")
    p, n = cases.physics("visc"), cases.numerics()
    part = fa.partition_rcb(m, 2)
    sp = fa.FlowFV(m, p, n, partition=part, rank=0)
    assert sp.nghost > 0
    du = torch.ones((sp.nown + sp.nghost, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="fvhip_comm_init"):
        sp.surface_data_device(du.data_ptr(), 2)
    with pytest.raises(RuntimeError, match="fvhip_comm_init"):
        sp.entropy_error_device(du.data_ptr())
    sp.close()
