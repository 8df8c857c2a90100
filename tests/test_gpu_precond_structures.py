"""The preconditioner structures real handles hold (lines, colouring, multigrid levels) and the solves that run
on them, against tests/fixtures/precond_structures.json: the cases of tests/test_precond_setup_host.py through
the handle API (fvhip_lines, fvhip_colouring, fvhip_amg_level), plus bitwise residual histories of 3-step
backward-Euler solves with every structure-dependent preconditioner. The packed lane arrays of the line solve
and the multigrid's Galerkin lists are not exposed by the API; a changed entry changes those histories (the
device path has no atomics: tests/test_gpu_implicit.py::test_resumed_solve_matches_one_call relies on the same
bitwise repeatability).

The fixture is written by this module's own collecting functions:
    PYTHONPATH=. python tests/test_gpu_precond_structures.py <commit> [out.json]
records what the checked-out tree computes as the behaviour of <commit>; the recorder refuses a recording that
misses the coverage table of test_precond_setup_host.CASES."""
import json
import sys

import numpy as np
import pytest

import fvens_amd as fa
import cases
from test_precond_setup_host import AMG_LEVELS, AMG_THRESHOLD, CASES, FIXTURE, check_coverage, fixture, summary

pytestmark = pytest.mark.gpu

# the solves of test_gpu_implicit.py::test_one_backward_euler_step_matches_host that depend on the structures:
# (prec_single, prec_gs, prec_lines, prec_ilu, prec_amg, cgs_refine)
HISTORIES = {
    "lines_fp64": (False, False, True, False, 0, 1),
    "lines_fp32": (True, False, True, False, 0, 1),
    "gauss_seidel": (False, True, False, False, 0, 1),
    "ilu0": (False, False, False, True, 0, 1),
    "amg_lines": (False, False, True, False, 3, 0),
}
HISTORY_CASE = "naca_ogrid"


def _numerics():
    return cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")


def collect(name):
    """summary (test_precond_setup_host.summary) of one case's handle"""
    import torch
    c = CASES[name]
    m, p, n = c["mesh"](), cases.physics(c["physics"]), _numerics()
    thr = c["thr"] if c["thr"] > 0 else 4.0
    others, grp = [], None
    if "nparts" in c:
        # a rank's hierarchy is built by a group solve (a lone partitioned handle has no exchange): one step
        # without a linear iteration sets the preconditioner up on every rank
        from test_gpu_implicit import _partitioned
        sps, dus, _ = _partitioned(m, p, n, cases.state(m, p, 8), c["nparts"])
        dev = sps[c["rank"]]
        others = [s for s in sps if s is not dev]
        grp = fa.FlowFVGroup(sps)
    else:
        dev = fa.FlowFV(m, p, n)
    lines = dev.lines(c["thr"])
    start = np.concatenate([[0], np.cumsum([len(cl) for cl, _ in lines])])
    cells, faces = np.concatenate([cl for cl, _ in lines]), np.concatenate([f for _, f in lines])
    colour, triples = dev.colouring()
    if grp is not None:
        cfg = fa.ImplicitConfig(cflinit=5.0, cflfin=5.0, tol=0.0, maxiter=1, lin_maxit=0, prec_lines=True,
                                line_threshold=thr, prec_amg=AMG_LEVELS, amg_threshold=AMG_THRESHOLD)
        grp.steady_backward_euler_device([d.data_ptr() for d in dus], cfg)
        nlev = 0
        while True:
            try:
                dev.amg_level(nlev + 1)
            except RuntimeError:
                break
            nlev += 1
    else:
        # block-diagonally dominant blocks: the hierarchy depends on the mesh alone
        rng = np.random.default_rng(7)
        N, Fi = m.nelem, m.naface - m.nbface
        D = rng.standard_normal((N, 4, 4)) + 16.0 * np.eye(4)[None]
        lo, up = 0.5 * rng.standard_normal((Fi, 4, 4)), 0.5 * rng.standard_normal((Fi, 4, 4))
        held = [torch.tensor(a.reshape(-1, 16), device="cuda") for a in (D, lo, up)]
        nlev = dev.amg_precondition_device(*[t.data_ptr() for t in held], levels=AMG_LEVELS, threshold=AMG_THRESHOLD,
                                           line_threshold=thr)
    levels = [dev.amg_level(l) for l in range(1, nlev + 1)]
    s = summary(dev.nown, dev.nghost, start, cells, faces, colour, triples, levels)
    if grp is not None:
        grp.close()
    for d in [dev] + others:
        d.close()
    return s


def history(key):
    """residual history of 3 backward-Euler steps on HISTORY_CASE, as float.hex() strings"""
    import torch
    single, gs, lines, ilu, amg, refine = HISTORIES[key]
    c = CASES[HISTORY_CASE]
    m, p, n = c["mesh"](), cases.physics(c["physics"]), _numerics()
    dev = fa.FlowFV(m, p, n)
    dU = torch.tensor(np.ascontiguousarray(cases.state(m, p, 8)[dev.permutation()]), device="cuda")
    cfg = fa.ImplicitConfig(cgs_refine=refine, cflinit=5.0, cflfin=5.0, tol=0.0, maxiter=3, lin_rtol=1e-13, lin_maxit=3000,
                            restart=60, prec_sweeps=1 if amg else 2, min_relax=1.0, prec_single=single, prec_gs=gs,
                            prec_lines=lines, prec_ilu=ilu, prec_amg=amg)
    st, hist = dev.steady_backward_euler_device(dU.data_ptr(), cfg)
    dev.close()
    assert st["steps"] == 3
    return [float(x).hex() for x in hist]


@pytest.mark.parametrize("name", list(CASES))
def test_handle_structures_match_recording(name):
    s = collect(name)
    check_coverage(name, s)
    assert s == fixture()["cases"][name]


@pytest.mark.parametrize("key", list(HISTORIES))
def test_solve_history_is_bitwise_the_recorded_one(key):
    assert history(key) == fixture()["histories"][key]


if __name__ == "__main__":
    commit = sys.argv[1]
    out = {"recorded_from_commit": commit, "amg_levels": AMG_LEVELS, "amg_threshold": AMG_THRESHOLD, "cases": {},
           "histories": {}}
    for name in CASES:
        out["cases"][name] = collect(name)
        print(name, json.dumps(out["cases"][name]), flush=True)
        check_coverage(name, out["cases"][name])
    for key in HISTORIES:
        out["histories"][key] = history(key)
        print(key, out["histories"][key], flush=True)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
