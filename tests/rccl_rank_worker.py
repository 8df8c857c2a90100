#!/usr/bin/env python3
"""One rank of tests/test_gpu_rccl_ranks.py: N processes on ONE GPU drive the library's own RCCL
communicator through its real multi-rank legs (ncclSend/ncclRecv halo exchange inside
ncclGroupStart/End, ncclAllReduce of the Krylov dot products and norms, ncclMin of the TVD-RK step).

RCCL refuses two ranks on one device ("Duplicate GPU detected", keyed by host hash and bus id), so each
rank sets its own NCCL_HOSTID: RCCL then sees N hosts and moves the data over its socket transport on
the loopback interface -- slow, but the library's calls, their pairing and their ordering are exactly
those of the one-GPU-per-rank run. torch.distributed (gloo) only rendezvouses the ranks and carries the
RCCL unique id and the results; the single-GPU reference results are computed by every rank itself.

usage (set by the test): RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT, NCCL_HOSTID in the environment;
argv: <out.json> <mesh key> <partitioner> [numerics]  (numerics: "visc" = laminar Roe + WLS + Van Albada +
Sutherland, "venkat" = Roe + WLS + Venkatakrishnan; "amg" = the implicit steps preconditioned by the multigrid
(prec_amg 3) and the rank's V-cycle against the group's, without the residual and TVD-RK legs the other rows cover;
"functionals" = the surface functionals of markers 2 and 4 and the entropy error over the communicator -- the
ncclAllReduce that stands for the reference's mpi_all_reduce at flow_spatial.cpp:303 and aoutput.cpp:50 -- laminar at
3 degrees, beside the one-handle results the rank computes itself, without the residual, implicit and TVD-RK legs)
partitioner: "graph", "rcb", or "rings" = three bands of equal cell counts by the distance of the cell centre from
the body, so that rank 0 holds every wall face, rank 2 every far-field face and rank 1 no face of either marker
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def amg_cycles(fa, torch, cases, m, p, n, part, sp, g, rank, world):
    """the rank's V-cycle through the single-handle call (its finest residuals exchange over RCCL) against the rows
    of this rank in the in-process group's V-cycle, on blocks both assemble themselves (CFL 20, state seed 4):
    per case the number of owned rows whose bits differ and the largest difference relative to max|z|"""
    def blocks(h, du, dt):
        st = h.layout_stats()
        Fi = max(st["faces"] - st["bfaces"], 1)
        blk = [torch.zeros((k, 16), dtype=torch.float64, device="cuda") for k in (h.nown, Fi, Fi)]
        torch.cuda.synchronize()
        h.assemble_jacobian_device(du.data_ptr(), *[t.data_ptr() for t in blk])
        h.add_pseudo_time_term_device(20.0, dt.data_ptr(), blk[0].data_ptr())
        h.synchronize()
        return blk

    def state(h, gk):
        du = torch.full((h.nown + h.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
        du[:h.nown] = torch.tensor(u[gk], device="cuda")
        return du, torch.zeros((h.nown, 4), dtype=torch.float64, device="cuda"), \
            torch.zeros(h.nown, dtype=torch.float64, device="cuda")

    u = cases.state(m, p, seed=4)
    v = np.random.default_rng(17).standard_normal((m.nelem, 4))
    du, dr, dt = state(sp, g)
    torch.cuda.synchronize()
    sp.compute_residual_device(du.data_ptr(), dr.data_ptr(), dt.data_ptr(), True, True)
    sp.synchronize()
    mine = blocks(sp, du, dt)
    sps = [fa.FlowFV(m, p, n, partition=part, rank=k) for k in range(world)]
    gs = [np.nonzero(part == k)[0][s_.permutation()] for k, s_ in enumerate(sps)]
    sts = [state(s_, gs[k]) for k, s_ in enumerate(sps)]
    torch.cuda.synchronize()
    grp = fa.FlowFVGroup(sps)
    grp.compute_residual_device(*[[t[j].data_ptr() for t in sts] for j in range(3)], True)
    theirs = [blocks(s_, sts[k][0], sts[k][2]) for k, s_ in enumerate(sps)]
    out = {}
    for name, lt, smoother, rows in (("pbj_gs", 0.0, 0, 0), ("lines_bjgs64", 4.0, 1, 64)):
        kw = dict(levels=3, threshold=0.2, sweeps=2, coarse_sweeps=6, line_threshold=lt, smoother=smoother, block_rows=rows)
        dv, dz = torch.tensor(v[g], device="cuda"), torch.full((sp.nown, 4), float("nan"), dtype=torch.float64, device="cuda")
        dvs = [torch.tensor(v[gk], device="cuda") for gk in gs]
        dzs = [torch.full((s_.nown, 4), float("nan"), dtype=torch.float64, device="cuda") for s_ in sps]
        torch.cuda.synchronize()
        sp.amg_precondition_smoother_device(*[t.data_ptr() for t in mine], d_v=dv.data_ptr(), d_z=dz.data_ptr(), **kw)
        grp.amg_precondition_device(*[[b[j].data_ptr() for b in theirs] for j in range(3)],
                                    d_vs=[t.data_ptr() for t in dvs], d_zs=[t.data_ptr() for t in dzs], **kw)
        z, zg = dz.cpu().numpy(), dzs[rank].cpu().numpy()
        out[name] = {"finite": bool(np.isfinite(z).all() and np.isfinite(zg).all()),
                     "rows_differing": int((z != zg).any(axis=1).sum()),
                     "rel": float(np.abs(z - zg).max() / np.abs(zg).max())}
    grp.close()
    for s_ in sps:
        s_.close()
    return out


def partition_rings(m, world):
    """bands of equal cell counts by the distance of the cell centre from the nearest face centre of marker 2.
    (The distance from a point does not order the layers of an O-grid round a slender body: about mid-chord the
    leading- and trailing-edge wall cells lie farther out than the fourteenth layer at mid-chord.)"""
    wall = np.asarray(m.gr).reshape(-1, 2)[np.nonzero(np.asarray(m.btags).reshape(m.nbface, -1)[:, 0] == 2)[0]]
    rc = np.asarray(m.rc)[:m.nelem]
    d = np.sqrt(((rc[:, None, :] - wall[None, :, :]) ** 2).sum(2)).min(1)
    part = np.empty(m.nelem, np.int32)
    part[np.argsort(d, kind="stable")] = (np.arange(m.nelem) * world) // m.nelem
    return part


def functionals(torch, cases, m, p, one, sp, g):
    """markers 2 and 4 and the entropy error on the communicator and on the one handle (state seed 31; the rank's
    ghost rows start as NaN). Floats go through JSON by repr, which round-trips every bit."""
    u = cases.state(m, p, seed=31)
    du1 = torch.tensor(np.ascontiguousarray(u[one.permutation()]), device="cuda")
    du = torch.full((sp.nown + sp.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
    du[:sp.nown] = torch.tensor(u[g], device="cuda")
    torch.cuda.synchronize()
    out = {}
    for marker in (2, 4):
        f1, rows1 = one.surface_data_device(du1.data_ptr(), marker)
        f, rows = sp.surface_data_device(du.data_ptr(), marker)
        out["marker%d" % marker] = {"funcs": list(f), "rows": rows.tolist(), "one_funcs": list(f1),
                                    "one_rows": rows1.tolist()}
    out["entropy"] = sp.entropy_error_device(du.data_ptr())
    out["one_entropy"] = one.entropy_error_device(du1.data_ptr())
    return out


def main():
    out_path, meshkey, partitioner = sys.argv[1], sys.argv[2], sys.argv[3]
    mode = sys.argv[4] if len(sys.argv) > 4 else ""

    def mark(msg):
        print("[rank %s] %s" % (os.environ["RANK"], msg), flush=True)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="env://")
    torch.cuda.set_device(0)
    import fvens_amd as fa
    import cases
    from test_gpu_residual import get_mesh

    m, _ = get_mesh(meshkey)
    p = cases.physics("visc", aoa_deg=3.0) if mode == "functionals" else cases.physics("visc" if mode == "visc" else "naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VENKATAKRISHNAN" if mode == "venkat" else "VANALBADA")
    if partitioner == "rings":
        part = partition_rings(m, world)
        # before the first collective, from what every rank holds: who owns the faces of each marker
        tags = np.asarray(m.btags).reshape(m.nbface, -1)[:, 0]
        held = {k: np.bincount(part[m.intfac[np.nonzero(tags == k)[0], 0]], minlength=world) for k in (2, 4)}
        assert world == 3 and held[2][1] == held[2][2] == 0 and held[4][0] == held[4][1] == 0, held
        assert held[2][0] == (tags == 2).sum() > 0 and held[4][2] == (tags == 4).sum() > 0, held
        assert np.bincount(part, minlength=world).tolist() == [m.nelem // world] * world
    else:
        part = fa.partition_graph(m, world, weights="cost") if partitioner == "graph" else fa.partition_rcb(m, world)
    amg = mode == "amg"
    # before the first collective, from the partition every rank holds: a rank whose cells do not coarsen would
    # throw inside the solve while the others wait in an allreduce
    assert not amg or np.bincount(part, minlength=world).min() >= 128, np.bincount(part, minlength=world)

    def uid():
        obj = [fa.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        return obj[0]

    if os.environ.get("FVHIP_CRASHTRACE"):
        # diagnostic: native backtrace of a crash (tools/probes/crashtrace.c), installed after every
        # library that might set its own handlers has loaded
        import ctypes
        ctypes.CDLL(os.environ["FVHIP_CRASHTRACE"])
        mark("crash tracer installed")
    rep = {"rank": rank, "world": world}
    owned = np.nonzero(part == rank)[0]
    mark("mesh and partition ready")

    # 1. residuals: five back-to-back partitioned residuals on changing states, each owned row bitwise
    #    the single-GPU residual (ghost rows start as NaN: a missed exchange cannot pass)
    one = fa.FlowFV(m, p, n)
    sp = fa.FlowFV(m, p, n, partition=part, rank=rank)
    sp.comm_init(world, rank, uid())
    g = owned[sp.permutation()]
    p1 = one.permutation()
    if mode == "functionals":
        rep["layout"] = sp.layout_stats()
        rep["functionals"] = functionals(torch, cases, m, p, one, sp, g)
        mark("functionals done")
        sp.close()
        one.close()
        with open(out_path, "w") as f:
            json.dump(rep, f)
        dist.barrier()
        dist.destroy_process_group()
        return
    bad = 0
    for k in range(0 if amg else 5):
        u = cases.state(m, p, seed=20 + k)
        du1 = torch.tensor(u[p1], device="cuda")
        dr1 = torch.zeros_like(du1)
        dt1 = torch.zeros(m.nelem, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()  # torch's stream vs the library's (non-blocking) streams
        one.compute_residual_device(du1.data_ptr(), dr1.data_ptr(), dt1.data_ptr(), True, True)
        one.synchronize()                 # the library's stream, not torch's
        r1 = np.empty((m.nelem, 4))
        t1 = np.empty(m.nelem)
        r1[p1] = dr1.cpu().numpy()
        t1[p1] = dt1.cpu().numpy()
        du = torch.full((sp.nown + sp.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
        du[:sp.nown] = torch.tensor(u[g], device="cuda")
        dr = torch.zeros((sp.nown, 4), dtype=torch.float64, device="cuda")
        dt = torch.zeros(sp.nown, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sp.compute_residual_device(du.data_ptr(), dr.data_ptr(), dt.data_ptr(), True, True)
        sp.synchronize()
        bad += int((dr.cpu().numpy() != r1[g]).any(axis=1).sum() + (dt.cpu().numpy() != t1[g]).sum())
    rep["residual_mismatched_rows"] = bad
    rep["layout"] = sp.layout_stats()
    mark("residuals done")

    # 2. implicit steps (GMRES dot products and norms through ncclAllReduce; block-Jacobi across ranks
    #    for the line preconditioner): the same steps as a one-process group of the same partition
    u0 = cases.state(m, p, seed=8)
    for lines in (False, True):
        cfg = fa.ImplicitConfig(cflinit=10.0, cflfin=200.0, tol=0.0, maxiter=3, lin_rtol=1e-4, lin_maxit=60,
                                restart=20, prec_sweeps=2 if not (lines or amg) else 1, min_relax=0.2, prec_lines=lines,
                                prec_amg=3 if amg else 0)
        du = torch.full((sp.nown + sp.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
        du[:sp.nown] = torch.tensor(u0[g], device="cuda")
        torch.cuda.synchronize()
        st, hist = sp.steady_backward_euler_device(du.data_ptr(), cfg)
        sp.synchronize()
        ur = du[:sp.nown].cpu().numpy()
        # the in-process group of the same partition (device copies, host sums), on rank 0's view
        sps = [fa.FlowFV(m, p, n, partition=part, rank=k) for k in range(world)]
        dus = []
        for k, s_ in enumerate(sps):
            gk = np.nonzero(part == k)[0][s_.permutation()]
            d = torch.full((s_.nown + s_.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
            d[:s_.nown] = torch.tensor(u0[gk], device="cuda")
            dus.append(d)
        torch.cuda.synchronize()
        grp = fa.FlowFVGroup(sps)
        stg, histg = grp.steady_backward_euler_device([d.data_ptr() for d in dus], cfg)
        for s_ in sps:
            s_.synchronize()
        ug = dus[rank][:sps[rank].nown].cpu().numpy()
        grp.close()
        for s_ in sps:
            s_.close()
        scale = np.abs(u0[g] - ug).max()
        key = "implicit_lines" if lines else "implicit_pbj"
        rep[key] = {"steps": st["steps"], "lin_iters": st["lin_iters"], "group_lin_iters": stg["lin_iters"],
                    "hist_rel": float(np.max(np.abs(np.asarray(hist) - np.asarray(histg)) / np.abs(histg))),
                    "u_rel": float(np.abs(ur - ug).max() / scale)}
        mark("implicit %s done" % key)

    if amg:
        rep["cycle"] = amg_cycles(fa, torch, cases, m, p, n, part, sp, g, rank, world)
        mark("V-cycles done")
        sp.close()
        one.close()
        with open(out_path, "w") as f:
            json.dump(rep, f)
        dist.barrier()
        dist.destroy_process_group()
        return

    # 3. TVD-RK: the global dtmin through ncclMin, bitwise the one-GPU steps
    mark("tvdrk")
    u0 = cases.state(m, p, seed=9)
    du1 = torch.tensor(u0[p1], device="cuda")
    torch.cuda.synchronize()
    s1, t1 = one.tvdrk_device(du1.data_ptr(), 3, 0.4, 1e9, 3)
    one.synchronize()
    uo = np.empty_like(u0)
    uo[p1] = du1.cpu().numpy()
    du = torch.full((sp.nown + sp.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
    du[:sp.nown] = torch.tensor(u0[g], device="cuda")
    torch.cuda.synchronize()
    s, t = sp.tvdrk_device(du.data_ptr(), 3, 0.4, 1e9, 3)
    sp.synchronize()
    rep["tvdrk"] = {"steps": s, "time_equal": t == t1,
                    "mismatched_rows": int((du[:sp.nown].cpu().numpy() != uo[g]).any(axis=1).sum())}
    sp.close()
    one.close()
    with open(out_path, "w") as f:
        json.dump(rep, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
