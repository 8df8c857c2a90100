"""Host-only checks of the fused residual's per-patch records (layout.hpp FzPatchRec, no GPU): building
the layout runs buildFused's self-check, which decodes every record with the kernel's own decoder and
compares it with the six per-patch arrays it packs, and asserts that every ghost gradient row holds four
0xFFFF neighbour codes (the invariant that lets the kernel load a row's codes without testing its cell).
A layout that builds has passed it; fvhip_layout_probe is the entry tests/test_layout.py uses."""
import pytest

import fvens_amd as fa
import cases

# (mesh, physics kind of the inviscid numerics, of the viscous ones): the kinds carry the meshes' markers
MESHES = {"naca_ogrid_96_6_18": (lambda: fa.UMesh.naca_ogrid(96, 6, 18), "naca", "visc"),
          "2dcylinderhybrid": (lambda: fa.UMesh.read_gmsh(cases.fixture_mesh("2dcylinderhybrid")), "cyl", "visc"),
          "naca0012luo": (lambda: fa.UMesh.read_gmsh(cases.fixture_mesh("naca0012luo")), "naca", "visc"),
          "flat_plate_48_32": (lambda: fa.UMesh.flat_plate(48, 32), "plate_inviscid", "plate"),
          "cylinder_ogrid_64_40": (lambda: fa.UMesh.cylinder_ogrid(64, 40), "cyl", "visc")}
# Roe/WLS/Van Albada, Roe/WLS/Venkatakrishnan, the viscous linear numerics (Roe/WLS/unlimited linear)
NUMERICS = {"vanalbada": (False, "VANALBADA"), "venkatakrishnan": (False, "VENKATAKRISHNAN"),
            "viscous_linear": (True, "NONE")}

# the smallest generator mesh (searched on the host over naca_ogrid, flat_plate and cylinder_ogrid sizes up
# to 28,672 cells) with a patch that stages more rows than its block has threads: 4,200 cells, one such
# patch of 257 rows; the second has three, of up to 275 rows
OVER_BLOCK_MESH = (100, 6, 18)
OVER_BLOCK_MESH_2 = (112, 8, 24)

_meshes = {}


def _mesh(key):
    if key not in _meshes:
        _meshes[key] = MESHES[key][0]()
    return _meshes[key]


@pytest.mark.parametrize("numerics", list(NUMERICS))
@pytest.mark.parametrize("meshkey", list(MESHES))
def test_fused_records_pass_the_builders_self_check(meshkey, numerics):
    viscous, rec = NUMERICS[numerics]
    m = _mesh(meshkey)
    p = cases.physics(MESHES[meshkey][2 if viscous else 1])
    st = fa.layout_probe(m, p, cases.numerics("ROE", "LEASTSQUARES", rec))     # raises if the self-check fails
    assert st["cells"] == m.nelem and st["patches"] > 0
    # a fused layout: the records exist and were checked
    assert st["max_staged_cells"] > 0 and st["ring1_cells"] > 0, st
    assert st["max_staged_cells"] <= 0xFFFF and st["max_slots"] <= 0xFFFF


@pytest.mark.parametrize("dims", [OVER_BLOCK_MESH, OVER_BLOCK_MESH_2])
@pytest.mark.parametrize("rec", ["VANALBADA", "VENKATAKRISHNAN"])
def test_over_block_mesh_stages_a_second_round(dims, rec):
    """the mesh tests/test_gpu_fused_prologue.py runs for the two-round staging path has such a patch"""
    m = fa.UMesh.naca_ogrid(*dims)
    st = fa.layout_probe(m, cases.physics("naca"), cases.numerics("ROE", "LEASTSQUARES", rec))
    assert st["patches_over_block"] > 0, st
    assert st["max_staged_cells"] > st["slots_per_patch"], st
