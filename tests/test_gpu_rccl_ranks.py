"""The library's multi-rank RCCL legs on ONE GPU (tests/rccl_rank_worker.py): N processes, one rank
each, every rank with its own NCCL_HOSTID so RCCL accepts them on the same device and routes them over
its socket transport on the loopback interface. What runs is the real partitioned path of the driver's
multi-GPU bench -- the two-layer halo exchanged by ncclSend/ncclRecv pairs inside ncclGroupStart/End on
the comm stream, overlapped with the interior patches; ncclAllReduce of the GMRES dot products and the
residual norms; ncclMin of the TVD-RK time step -- checked against one GPU:
  * five back-to-back residuals on changing states: every owned row and time step bitwise;
  * three implicit steps (point-block Jacobi, and the line-implicit preconditioner whose lines are cut
    at rank boundaries): the same linear iterations, residual history and states as the in-process group
    of the same partition (rounding of the dot-product sums aside: 1e-9);
  * TVD-RK order 3: bitwise the one-GPU steps and time;
  * mode "amg" (3 ranks): the implicit steps preconditioned by the multigrid (prec_amg 3; point-block and line
    finest smoother) to the same bars, and the rank's V-cycle through the single-handle call -- its finest
    residuals exchange the iterate over RCCL -- bit for bit the rows of that rank in the in-process group's
    V-cycle (the same kernels on the same data; measured: no row differs on any rank, either case);
  * mode "functionals" (3 ranks, partition "rings": rank 0 holds every wall face, rank 2 every far-field face, rank 1
    none of either): the surface functionals of both markers and the entropy error through ncclAllReduce -- the same
    bits on every rank, the ranks' face rows a permutation of the one handle's bit for bit, the sums within the
    worst-case bound of adding the same terms in another order. A second row runs the mode on the graph
    partition, where every rank holds faces of each marker and the all-reduce adds real terms.
(Round 4's hipGraph capture of the rank step was removed in round 5: RCCL's captured p2p group overflows
the stack in the HIP runtime's graph code, profiles/r05/graph_capture_crash.txt.)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, meshkey, partitioner, mode=""):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), NCCL_HOSTID="fvhip-rank-%d" % r, NCCL_SOCKET_IFNAME="lo",
                   NCCL_IB_DISABLE="1")
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "rccl_rank_worker.py"),
                                       str(tmp_path / ("r%d.json" % r)), meshkey, partitioner] + ([mode] if mode else []),
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=240)
            logs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed (%d):\n%s" % (r, p.returncode, logs[r][-3000:])
    reps = [json.load(open(tmp_path / ("r%d.json" % r))) for r in range(world)]
    print(json.dumps(reps))
    return reps


@pytest.mark.parametrize("world,meshkey,partitioner,numerics", [(2, "naca_small", "graph", ""), (4, "naca_small", "rcb", ""),
                                                              (3, "naca_small", "graph", "visc"),
                                                              (3, "naca_small", "graph", "venkat"),
                                                              (3, "naca_small", "graph", "amg"),
                                                              (3, "naca_small", "rings", "functionals"),
                                                              (3, "naca_small", "graph", "functionals")])
def test_rccl_ranks_on_one_gpu(tmp_path, world, meshkey, partitioner, numerics):
    """the headline numerics on 2 and 4 ranks; BASELINE config 5's (laminar, Sutherland: the fused viscous
    kernel on the two-layer halo) and config 4's (Venkatakrishnan: the layer-1 ghosts' limiter values
    formed locally) on 3 ranks; the multigrid (config 5's preconditioner) on 3 ranks"""
    reps = _run_ranks(tmp_path, world, meshkey, partitioner, numerics)
    for rep in reps:
        assert rep["layout"]["neighbours"] > 0 and rep["layout"]["ghosts"] > 0
    if numerics == "functionals":
        _check_functionals([rep["functionals"] for rep in reps], meshkey, rings=partitioner == "rings")
        return
    for rep in reps:
        if numerics == "amg":
            for key in ("implicit_pbj", "implicit_lines"):
                im = rep[key]
                assert im["steps"] == 3 and im["lin_iters"] == im["group_lin_iters"], (key, im)
                assert im["hist_rel"] <= 1e-9 and im["u_rel"] <= 1e-9, (key, im)
            for key in ("pbj_gs", "lines_bjgs64"):
                assert rep["cycle"][key]["finite"] and rep["cycle"][key]["rows_differing"] == 0, (key, rep["cycle"][key])
            continue
        assert rep["residual_mismatched_rows"] == 0, rep
        for key in ("implicit_pbj", "implicit_lines"):
            im = rep[key]
            assert im["steps"] == 3 and im["lin_iters"] == im["group_lin_iters"], (key, im)
            assert im["hist_rel"] <= 1e-9 and im["u_rel"] <= 1e-9, (key, im)
        assert rep["tvdrk"]["steps"] == 3 and rep["tvdrk"]["time_equal"] and rep["tvdrk"]["mismatched_rows"] == 0


def _check_functionals(fs, meshkey, rings):
    """the "functionals" row: the reports of the three ranks against each other, against the one-handle results every
    rank computed itself and against the long-double restatement (tests/functionals_host.py); rings: the partition
    that puts each marker on one rank, else the one that shares both markers between ranks"""
    import _oracle as orc
    import cases
    import functionals_host as fh
    from test_gpu_residual import get_mesh
    m, om = get_mesh(meshkey)
    p, n = cases.physics("visc", aoa_deg=3.0), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u = cases.state(m, p, seed=31)
    grads = orc.OracleSpatial(om, p, n).getGradients(u)
    nranks = len(fs)
    u53 = 2.0 ** -53
    for marker in (2, 4):
        key = "marker%d" % marker
        funcs = np.array([f[key]["funcs"] for f in fs])
        one = np.array(fs[0][key]["one_funcs"])
        one_rows = np.array(fs[0][key]["one_rows"]).reshape(-1, 4)
        assert all(f[key]["one_funcs"] == fs[0][key]["one_funcs"] and f[key]["one_rows"] == fs[0][key]["one_rows"]
                   for f in fs)
        # the all-reduce result is the same everywhere
        assert np.isfinite(funcs).all() and (funcs == funcs[0]).all(), funcs
        # the per-rank face lists: rank 1 has none, and together they are the one handle's rows bit for bit
        counts = [len(f[key]["rows"]) for f in fs]
        nface = len(one_rows)
        assert sum(counts) == nface == len(fh.marker_faces(m, marker)), counts
        if rings:
            assert counts == ([nface, 0, 0] if marker == 2 else [0, 0, nface]), counts
        else:
            assert sum(c > 0 for c in counts) >= 2, counts
        rows = np.array([r for f in fs for r in f[key]["rows"]]).reshape(-1, 4)
        where = {(x, y): i for i, (x, y) in enumerate(one_rows[:, :2].tolist())}
        assert len(where) == nface
        at = [where[(x, y)] for x, y in rows[:, :2].tolist()]          # KeyError: a centre the one handle has not
        assert sorted(at) == list(range(nface))
        assert np.array_equal(rows, one_rows[at])
        # the sums: the same n terms in another order, over a length summed the same way
        prods = fh.surface_rows(m, p, u, grads, marker)[1]
        tot = float(fh.fsum(prods[:, 3]))
        for k, name in enumerate(("CL", "CDp", "CDsf")):
            bound = 4 * nface * u53 * float(fh.fsum(np.abs(prods[:, k]))) / tot
            print("ranks (%s) marker %d %s: faces per rank %s, |ranks - one handle| %.3g, bound %.3g (%.3g of it)"
                  % ("rings" if rings else "graph", marker, name, counts, abs(funcs[0][k] - one[k]), bound, abs(funcs[0][k] - one[k]) / bound))
            assert abs(funcs[0][k] - one[k]) <= bound, (marker, name, funcs[0][k], one[k])
    ent = [f["entropy"] for f in fs]
    one = fs[0]["one_entropy"]
    want = float(fh.entropy_error(m, p, u))
    print("ranks (%s) entropy: ranks - long double %.3g relative, ranks^2 - handle^2 %.3g relative"
          % ("rings" if rings else "graph", abs(ent[0] - want) / want, abs(ent[0] ** 2 - one ** 2) / one ** 2))
    assert all(e == ent[0] for e in ent) and all(f["one_entropy"] == one for f in fs), ent
    assert abs(ent[0] - want) <= 1e-12 * want and abs(one - want) <= 1e-12 * want, (ent[0], one, want)
    assert abs(ent[0] ** 2 - one ** 2) <= 4 * nranks * u53 * one ** 2, (ent[0], one)
