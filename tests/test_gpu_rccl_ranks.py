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
    V-cycle (the same kernels on the same data; measured: no row differs on any rank, either case).
(Round 4's hipGraph capture of the rank step was removed in round 5: RCCL's captured p2p group overflows
the stack in the HIP runtime's graph code, profiles/r05/graph_capture_crash.txt.)
"""
import json
import os
import subprocess
import sys

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
                                                              (3, "naca_small", "graph", "amg")])
def test_rccl_ranks_on_one_gpu(tmp_path, world, meshkey, partitioner, numerics):
    """the headline numerics on 2 and 4 ranks; BASELINE config 5's (laminar, Sutherland: the fused viscous
    kernel on the two-layer halo) and config 4's (Venkatakrishnan: the layer-1 ghosts' limiter values
    formed locally) on 3 ranks; the multigrid (config 5's preconditioner) on 3 ranks"""
    for rep in _run_ranks(tmp_path, world, meshkey, partitioner, numerics):
        assert rep["layout"]["neighbours"] > 0 and rep["layout"]["ghosts"] > 0
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
