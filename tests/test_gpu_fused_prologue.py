"""The head of the one-launch fused residual (k_residual_wls): the per-patch record replaces six arrays'
per-patch entries, the first loads of a block are issued together, and a gradient row's neighbour codes
are loaded without testing whether its cell is owned (a ghost row holds four 0xFFFF codes). None of this
changes an operation, so every result stays BITWISE what the staged kernels, the oracle and the single
handle give -- on a mesh with patches that stage more rows than the block has threads (the two-round
staging path), on a three-rank partition (ghost gradient rows, patch lists) and in the matrix-free operator
(the instantiations without time steps share the head)."""
import numpy as np
import pytest

import fvens_amd as fa
import _oracle as orc
import cases
from test_gpu_partition import run_partitioned
from test_gpu_residual import get_mesh
from test_layout_fused_record import OVER_BLOCK_MESH, OVER_BLOCK_MESH_2

pytestmark = pytest.mark.gpu

_cache = {}


def _mesh(key):
    if key == "naca_small":
        return get_mesh("naca_small")
    if key not in _cache:
        m = fa.UMesh.naca_ogrid(*key)
        _cache[key] = (m, orc.OracleMesh.from_raw(m.raw()))
    return _cache[key]


@pytest.mark.parametrize("rec", ["VANALBADA", "VENKATAKRISHNAN"])
@pytest.mark.parametrize("meshkey", [OVER_BLOCK_MESH, OVER_BLOCK_MESH_2, "naca_small"], ids=str)
def test_fused_equals_staged_and_oracle_bitwise(meshkey, rec):
    import torch
    m, om = _mesh(meshkey)
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", rec)
    u = cases.state(m, p, 5)
    dev = fa.FlowFV(m, p, n)
    st = dev.layout_stats()
    assert st["patches"] > 1
    if meshkey != "naca_small":
        assert st["patches_over_block"] > 0, st         # the second staging round runs
    perm = dev.permutation()
    du = torch.tensor(u[perm], device="cuda")
    out = []
    for staged in (False, True):
        dr = torch.full((m.nelem, 4), float("nan"), dtype=torch.float64, device="cuda")
        dt = torch.full((m.nelem,), float("nan"), dtype=torch.float64, device="cuda")
        dev.compute_residual_device(du.data_ptr(), dr.data_ptr(), dt.data_ptr(), True, True, staged=staged)
        dev.synchronize()
        out.append((dr.cpu().numpy(), dt.cpu().numpy()))
    dev.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    # the oracle, in the mesh's own cell order (the device rows are in internal order: row i is cell perm[i])
    ref = orc.OracleSpatial(om, p, n)
    r0 = np.zeros((m.nelem, 4))
    dt0 = np.zeros(m.nelem)
    ref.compute_residual(u, r0, True, dt0)
    r = np.empty_like(r0)
    dtm = np.empty_like(dt0)
    r[perm] = out[0][0]
    dtm[perm] = out[0][1]
    np.testing.assert_array_equal(r, r0)
    np.testing.assert_array_equal(dtm, dt0)


@pytest.mark.parametrize("rec", ["VANALBADA", "VENKATAKRISHNAN"])
def test_three_rank_partition_bitwise(rec):
    """in-process three-rank partition with the two-layer halo: ghost cells are ring-1 (gradient) rows of
    the boundary patches, and every rank sweeps patch lists"""
    r, dt, r1, dt1, stats = run_partitioned("naca_small", "naca", "ROE", "LEASTSQUARES", rec, True, 3)
    assert all(s["ghosts"] > 0 and s["patches"] > 0 for s in stats), stats
    assert any(0 < s["interior_patches"] < s["patches"] for s in stats), stats
    np.testing.assert_array_equal(r, r1)
    np.testing.assert_array_equal(dt, dt1)


@pytest.mark.parametrize("rec", ["VANALBADA", "VENKATAKRISHNAN"])
def test_fused_matfree_operator_equals_three_launch_bitwise(rec):
    """the fused matrix-free operator (one launch of the residual kernel without time steps) against the
    three-launch operator a one-handle group runs"""
    import torch
    m, _ = get_mesh("naca_small")
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", rec)
    h1, h2 = fa.FlowFV(m, p, n), fa.FlowFV(m, p, n)
    grp = fa.FlowFVGroup([h2])
    perm = h1.permutation()
    rng = np.random.default_rng(3)
    du = torch.tensor(cases.state(m, p, 11)[perm], device="cuda")
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
    same = torch.equal(y1, y2)
    err = float((y1 - y2).abs().max())
    grp.close()
    h1.close()
    h2.close()
    assert bool(torch.isfinite(y1).all()) and float(y1.abs().max()) > 0
    assert same, err
