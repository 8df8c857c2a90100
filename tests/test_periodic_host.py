"""Periodic boundaries on the host: the restated compute_periodic_map (mesh.cpp:369-424) against the
reference's Mesh_Periodic known answer (tests/mesh/mesh.cpp:68-85, testperiodic.msh), the structure of the mesh
UMesh.periodic builds (paired faces become connectivity faces of the mesh with itself, in the reference's face
order), its refusals, and the layout a periodic handle would get. CPU only; the device path is
tests/test_gpu_periodic.py."""
import numpy as np
import pytest

import fvens_amd as fa
import cases


def _fixture():
    return fa.UMesh.read_gmsh(cases.fixture_mesh("testperiodic")), [(4, 0)]


MESHES = {
    "testperiodic": _fixture,
    "box4x3": lambda: (fa.UMesh.periodic_box(4, 3), [(4, 0)]),
    "box2x3_wrap": lambda: (fa.UMesh.periodic_box(2, 3, wrap_y=True), [(4, 0), (5, 1)]),
    "tri4x4_wrap_jitter": lambda: (fa.UMesh.periodic_box(4, 4, triangles=True, wrap_y=True, jitter=0.2),
                                   [(4, 0), (5, 1)]),
}


def test_periodic_map_reference_known_answer():
    """tests/mesh/mesh.cpp:68-85: faces 8..12 pair with 25..21 on testperiodic.msh, marker 4, axis 0"""
    m, _ = _fixture()
    pm = m.periodic_map(4, 0)
    assert pm.shape == (m.nbface,)
    for a, b in zip([8, 9, 10, 11, 12], [25, 24, 23, 22, 21]):
        assert pm[a] == b and pm[b] == a
    on = m.btags[:, 0] == 4
    assert on.sum() == 10
    assert (pm[~on] == -1).all()
    assert (pm[on] >= 0).all() and on[pm[on]].all()
    np.testing.assert_array_equal(pm[pm[on]], np.nonzero(on)[0])          # an involution on the marker's faces
    # what the reference's test asserts: each face's partner cell is the other face's interior cell
    for a, b in zip([8, 9, 10, 11, 12], [25, 24, 23, 22, 21]):
        assert m.intfac[a, 0] != m.intfac[b, 0]


@pytest.mark.parametrize("key", list(MESHES))
def test_periodic_mesh_structure(key):
    m, pairs = MESHES[key]()
    p = m.periodic(pairs)
    N = m.nelem
    pmap = np.full(m.nbface, -1, np.int32)
    for marker, axis in pairs:
        one = m.periodic_map(marker, axis)
        pmap = np.where(one >= 0, one, pmap)
    old = np.nonzero(pmap >= 0)[0]                 # old boundary faces that became connectivity faces, in order
    kept = np.nonzero(pmap < 0)[0]
    nc = len(old)
    assert nc > 0 and nc % 2 == 0
    # counts
    assert p.nelem == N and p.npoin == m.npoin
    assert p.nconnface == nc
    assert p.nbface + p.nconnface == m.nbface
    assert p.naface == m.naface and p.ninface == m.ninface
    # the remaining physical boundary faces first, in their old relative order
    nb = p.nbface
    np.testing.assert_array_equal(p.btags, m.btags[kept])
    np.testing.assert_array_equal(p.intfac[:nb, [0, 2, 3]], m.intfac[kept][:, [0, 2, 3]])
    np.testing.assert_array_equal(p.intfac[:nb, 1], N + nc + np.arange(nb))
    np.testing.assert_array_equal(p.rcbp, m.rcbp[kept])
    # interior faces unchanged
    np.testing.assert_array_equal(p.intfac[nb:nb + p.ninface], m.intfac[m.nbface:])
    np.testing.assert_array_equal(p.facemetric[nb:nb + p.ninface], m.facemetric[m.nbface:])
    np.testing.assert_array_equal(p.gr[nb:nb + p.ninface], m.gr[m.nbface:])
    # connectivity faces last, in old boundary-face order
    cf = p.intfac[nb + p.ninface:]
    np.testing.assert_array_equal(cf[:, 1], N + np.arange(nc))
    np.testing.assert_array_equal(cf[:, [0, 2, 3]], m.intfac[old][:, [0, 2, 3]])
    np.testing.assert_array_equal(p.connface[:, 0], cf[:, 0])
    assert (p.connface[:, 2] == -1).all()
    pos = {int(f): i for i, f in enumerate(old)}
    partner = np.array([pos[int(pmap[f])] for f in old])
    np.testing.assert_array_equal(partner[partner], np.arange(nc))
    assert (partner != np.arange(nc)).all()
    np.testing.assert_array_equal(p.connface[:, 3], p.connface[partner, 0])
    np.testing.assert_array_equal(p.connface[:, 4], np.minimum(old, pmap[old]))
    np.testing.assert_array_equal(p.connface[:, 4], p.connface[partner, 4])
    assert (p.connface[:, 3] != p.connface[:, 0]).all()
    # esuel / elemface renumbered to match
    for ic in range(nc):
        c, lf = p.connface[ic, 0], p.connface[ic, 1]
        assert p.esuel[c, lf] == N + ic and p.elemface[c, lf] == nb + p.ninface + ic
    for f in range(nb):
        c = p.intfac[f, 0]
        lf = int(np.nonzero(p.elemface[c, :p.nnode[c]] == f)[0][0])
        assert p.esuel[c, lf] == N + nc + f
    # ghost centres: the partner cell's centre displaced by the period
    assert p.rc.shape == (N + nc, 2)
    size = np.ptp(m.coords, axis=0).max()
    mid = p.gr[nb + p.ninface:]
    shift = p.rc[N:] - p.rc[p.connface[:, 3]]
    assert np.abs(shift - (mid - mid[partner])).max() <= 1e-14 * size
    assert (np.abs(shift).max(axis=1) > 0.5 * np.abs(mid - mid[partner]).max(axis=1)).all()
    # partners: equal lengths, opposite normals
    # (the bound periodic() itself enforces, 1e-8: the Gmsh fixture's points carry Gmsh's 1e-11 noise,
    # mesh.cpp:408; the generated boxes' boundary points are exact, so their partners agree to rounding)
    fm = p.facemetric[nb + p.ninface:]
    tol = 1e-8 if key == "testperiodic" else 4e-16
    assert np.abs(fm[:, 2] - fm[partner, 2]).max() <= tol * fm[:, 2].max()
    assert np.abs(fm[:, :2] + fm[partner, :2]).max() <= tol
    # cells and points untouched
    np.testing.assert_array_equal(p.area, m.area)
    np.testing.assert_array_equal(p.coords, m.coords)
    np.testing.assert_array_equal(p.rc[:N], m.rc)
    np.testing.assert_array_equal(p.inpoel, m.inpoel)


def test_box_generator_markers_and_jitter():
    a = fa.UMesh.periodic_box(4, 3, lx=2.0, ly=1.5)
    assert (a.nelem, a.nbface) == (12, 14)
    assert sorted(np.unique(a.btags[:, 0])) == [2, 3, 4]
    ymid = a.gr[:a.nbface, 1]
    assert (ymid[a.btags[:, 0] == 2] == 0.0).all() and (ymid[a.btags[:, 0] == 3] == 1.5).all()
    assert set(a.gr[:a.nbface, 0][a.btags[:, 0] == 4]) == {0.0, 2.0}
    b = fa.UMesh.periodic_box(4, 4, triangles=True, wrap_y=True, jitter=0.2)
    assert b.nelem == 32 and (b.nnode == 3).all() and sorted(np.unique(b.btags[:, 0])) == [4, 5]
    flat = fa.UMesh.periodic_box(4, 4, triangles=True, wrap_y=True)
    d = b.coords - flat.coords
    edge = (flat.coords[:, 0] == 0) | (flat.coords[:, 0] == 1) | (flat.coords[:, 1] == 0) | (flat.coords[:, 1] == 1)
    assert (d[edge] == 0).all() and (np.abs(d[~edge]).max(axis=1) > 0).all()
    assert np.abs(d).max() <= 0.2 * 0.25
    again = fa.UMesh.periodic_box(4, 4, triangles=True, wrap_y=True, jitter=0.2)
    np.testing.assert_array_equal(again.coords, b.coords)                  # seeded
    assert (b.area > 0).all()


def test_refuses_one_cell_across_the_period():
    m = fa.UMesh.periodic_box(1, 3)
    with pytest.raises(RuntimeError, match=r"boundary faces \d+ and \d+ belong to the same cell"):
        m.periodic([(4, 0)])


def test_refuses_an_odd_face_out(tmp_path):
    """a marker-4 face of a 3x2 box re-tagged in the Gmsh text: its former partner is left without one"""
    src = tmp_path / "box.msh"
    fa.UMesh.periodic_box(3, 2).write_gmsh(src)
    lines = src.read_text().splitlines()
    first = lines.index("$Elements") + 2
    hit = None
    for k in range(first, len(lines)):
        w = lines[k].split()
        if w[1] == "1" and w[3] == "4":           # a boundary edge of marker 4
            w[3] = "7"
            lines[k] = " ".join(w)
            hit = k - first
            break
    assert hit is not None
    dst = tmp_path / "odd.msh"
    dst.write_text("\n".join(lines) + "\n")
    m = fa.UMesh.read_gmsh(dst)
    pm = m.periodic_map(4, 0)
    on = np.nonzero(m.btags[:, 0] == 4)[0]
    lone = [int(f) for f in on if pm[f] < 0]
    assert len(on) == 3 and len(lone) == 1
    with pytest.raises(RuntimeError, match=rf"boundary face {lone[0]} of marker 4 has no partner"):
        m.periodic([(4, 0)])


def test_refuses_periodic_twice_and_partitioning():
    m = fa.UMesh.periodic_box(4, 3, wrap_y=True)
    p = m.periodic([(4, 0)])
    with pytest.raises(RuntimeError, match="already has connectivity faces"):
        p.periodic([(5, 1)])
    with pytest.raises(RuntimeError, match="global mesh"):
        p.restrict(fa.UMesh.partition_trivial(p.nelem, 2), 0)
    with pytest.raises(RuntimeError, match="single-domain mesh"):
        fa.partition_rcb(p, 2)
    with pytest.raises(RuntimeError, match="single-domain mesh"):
        fa.partition_graph(p, 2)
    with pytest.raises(RuntimeError, match="no boundary face carries marker 9"):
        m.periodic([(9, 0)])


@pytest.mark.parametrize("key", list(MESHES))
def test_layout_probe_of_a_periodic_mesh(key):
    m, pairs = MESHES[key]()
    p = m.periodic(pairs)
    phys = cases.physics("cyl")
    phys.bcconf = [fa.FlowBCConfig("farfield", int(t)) for t in np.unique(p.btags[:, 0])]
    st = fa.layout_probe(p, phys, cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
    assert st["cells"] == p.nelem and st["faces"] == p.naface and st["bfaces"] == p.nbface
    assert st["ghosts"] == p.nconnface
    assert st["neighbours"] == 1
    assert st["send_rows"] == p.nconnface


def test_mixed_self_and_rank_faces_are_refused():
    """a per-rank mesh view whose connectivity faces name rank -1 next to a real rank"""
    m = fa.UMesh.periodic_box(4, 3, wrap_y=True).periodic([(4, 0), (5, 1)])
    m.connface[0, 2] = 1
    keep = np.ascontiguousarray(m.connface)
    m.view.connface = keep.ctypes.data_as(fa._ffi.c_int_p)
    with pytest.raises(RuntimeError, match="periodic faces on a partitioned mesh are not supported"):
        fa.layout_probe(m, cases.physics("cyl"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
