#!/usr/bin/env python3
"""Secondary benchmark: device implicit pseudo-time steps (SteadyBackwardEulerSolver::solve,
aodesolver.cpp:363-638) on the bench mesh — residual + analytic first-order Jacobian + GMRES with
block-Jacobi sweeps + relaxed update per step, matrix-free and assembled operator.

Starts as the reference's transonic-implicit.ctrl does (freestream, first-order initialisation
solve), then times K second-order steps (tolerance 0 so every step runs) after W warm-up steps;
prints one JSON line per operator kind with ms/step, linear iterations per step and ms per linear
iteration. Not the headline metric (bench.py is); one GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


CASES = {   # physics, flux, gradients, reconstruction
    "naca": ("naca", "ROE", "LEASTSQUARES", "VANALBADA"),
    "naca-venkat": ("naca", "ROE", "LEASTSQUARES", "VENKATAKRISHNAN"),
    "plate": ("plate", "HLLC", "LEASTSQUARES", "NONE"),
    # testcases/visc-naca0012/laminar-implicit.ctrl: Roe, least squares, limiter none (:72), alpha 0 (:19)
    "visc-c5": ("visc", "ROE", "LEASTSQUARES", "NONE"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="naca", choices=sorted(CASES),
                    help="naca: bench.py's C4 workload; naca-venkat: BASELINE config 4 numerics on it; "
                         "plate: config 3, laminar flat plate, ~1M quads; visc-c5: config 5, laminar NACA0012, 8.1M cells")
    ap.add_argument("--scale", type=int, default=1, help="divide the mesh dimensions by this")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--init-steps", type=int, default=10, help="first-order initialisation steps")
    ap.add_argument("--cfl", type=float, default=25.0)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--lin-maxit", type=int, default=30)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--prec-single", action="store_true", help="preconditioner blocks in fp32")
    ap.add_argument("--gs", action="store_true", help="multicolour block Gauss-Seidel sweeps")
    ap.add_argument("--lines", action="store_true", help="line-implicit preconditioner")
    ap.add_argument("--ilu", action="store_true", help="block ILU(0) in multicolour order")
    ap.add_argument("--ilu-order", type=int, default=0,
                    help="with --ilu: sweep-based ILU(0)/SGS in a row order, 1 internal (Hilbert), 2 reverse Cuthill-McKee")
    ap.add_argument("--ilu-build", type=int, default=0, help="sweeps for its pivots (0: the SGS pivots)")
    ap.add_argument("--ilu-apply", type=int, default=0, help="sweeps per triangular solve")
    ap.add_argument("--ilu-table", action="store_true",
                    help="after the first-order start (with the options above), time the main steps from the same state "
                         "for point-block Jacobi (also with 4 block-Jacobi sweeps), the colour ILU, lines and the sweep-based ILU with (build, apply) = "
                         "(1,1), (2,2), (3,3), (3,5) and (0,2) in both orders: one line per operator and preconditioner")
    ap.add_argument("--repeat", type=int, default=1,
                    help="time the same steps this many times over (each from the same state) and report the mean")
    ap.add_argument("--kernel-times", action="store_true",
                    help="add the preconditioner kernels' mean times (event-timed in further steps after the timed ones)")
    ap.add_argument("--operators", default="assembled,matrix-free")
    ap.add_argument("--second-from", default="start", choices=["start", "freestream"])
    args = ap.parse_args()

    import torch
    torch.cuda.set_device(0)
    import fvens_amd as fa
    from bench import c4_mesh

    kind, flux, grad, rec = CASES[args.case]
    if kind == "plate":
        nx = ny = 1024 // args.scale
        mesh, dims = fa.UMesh.flat_plate(nx, ny), dict(nx=nx, ny=ny)
    elif args.case == "visc-c5":    # BASELINE config 5: laminar NACA0012, the 8,054,616-cell hybrid C5
        mesh, dims = c4_mesh(fa, args.scale, 2)
    else:
        mesh, dims = c4_mesh(fa, args.scale)
    for out in implicit_steps(mesh, args.case, steps=args.steps, warmup=args.warmup, init_steps=args.init_steps,
                              cfl=args.cfl, restart=args.restart, lin_maxit=args.lin_maxit, sweeps=args.sweeps,
                              single=args.prec_single, gs=args.gs, lines=args.lines, ilu=args.ilu,
                              operators=tuple(o == "matrix-free" for o in args.operators.split(",")),
                              second_from=args.second_from, ilu_order=args.ilu_order, ilu_build=args.ilu_build,
                              ilu_apply=args.ilu_apply, variants=ILU_TABLE if args.ilu_table else None,
                              kernel_times=args.kernel_times, repeat=args.repeat):
        out["dims"] = dims
        print(json.dumps(out), flush=True)


# --ilu-table: the preconditioners compared on one state (name, options over the command line's)
_OFF = dict(prec_gs=False, prec_lines=False, prec_ilu=False, ilu_order=0, ilu_build_sweeps=0, ilu_apply_sweeps=0)
ILU_TABLE = [("jacobi", _OFF), ("jacobi-4-sweeps", {**_OFF, "prec_sweeps": 4}), ("colour-ilu", {**_OFF, "prec_ilu": True}), ("lines", {**_OFF, "prec_lines": True})] + [
    ("order%d-b%d-a%d" % (o, b, a), {**_OFF, "prec_ilu": True, "ilu_order": o, "ilu_build_sweeps": b, "ilu_apply_sweeps": a})
    for o in (1, 2) for b, a in ((1, 1), (2, 2), (3, 3), (3, 5), (0, 2))]
PREC_KERNELS = ("k_bjac_apply", "k_bjac_sweep", "k_bjac_invert", "k_bgs_colour", "k_ilu_factor", "k_ilu_solve",
                "k_ilu_sweep_factor", "k_ilu_sweep_solve", "k_line_factor", "k_line_solve", "k_to_single", "k_block_apply")


def implicit_steps(mesh, case="naca", steps=5, warmup=2, init_steps=10, cfl=25.0, restart=30, lin_maxit=30,
                   sweeps=4, single=False, gs=False, operators=(False, True), lines=False, ilu=False,
                   init_cfl=None, part=None, rank=0, world=1, new_uid=None, allmax=None, second_from="start",
                   ilu_order=0, ilu_build=0, ilu_apply=0, variants=None, kernel_times=False, repeat=1):
    """time `steps` second-order backward-Euler steps per operator kind (False: assembled, True:
    matrix-free) after a first-order start; yields one dict per operator.
    second_from: "start" -- the second-order steps continue from the first-order start's state (the
    reference's two-stage schedule); "freestream" -- they start from the free stream themselves (the first
    second-order steps of a cold start, where the residual still falls; the first-order start is timed
    all the same)
    init_cfl: (cfl_min, cfl_max) of the first-order start's expResidualRamp (aodesolver.cpp:110-120,
    462; default: `cfl` held fixed). part/rank/world/new_uid: this rank's piece of a partition, its
    handles on the library's RCCL communicator (new_uid() -> a fresh unique id, the same on every rank);
    allmax(x): the maximum of x over ranks (the slowest rank's time)
    ilu_order / ilu_build / ilu_apply: the sweep-based ILU(0)/SGS (ImplicitConfig.ilu_order, ...; with ilu).
    variants: [(name, ImplicitConfig options)]: the main steps are timed once per entry, its options over the ones
    above, each from the same start state on the same handle (the first-order start uses the ones above); the
    record then carries "variant" and "prec" (a variant whose solve diverges is recorded as such and the table goes
    on). repeat: the timed steps run this many times, each from the same state, ms_per_step their mean. kernel_times: `warmup` further event-timed steps per record, the
    preconditioner kernels' mean ms per launch in "kernel_ms" (and the launch counts)"""
    import torch
    import fvens_amd as fa
    import cases
    kind, flux, grad, rec = CASES[case]
    p = cases.physics(kind)
    n = cases.numerics(flux, grad, rec)
    n1 = cases.numerics(flux, grad, rec, order2=False)
    dev = torch.cuda.current_device()
    kw = {} if part is None else dict(partition=part, rank=rank)

    def handle(nn):
        h = fa.FlowFV(mesh, p, nn, device=dev, **kw)
        if part is not None:
            h.comm_init(world, rank, new_uid())
        return h
    sp1 = handle(n1)
    sp = handle(n)
    perm = sp.permutation()
    assert np.array_equal(perm, sp1.permutation())
    nown = sp.nown if part is not None else mesh.nelem
    nrows = nown + (sp.nghost if part is not None else 0)
    u0 = np.zeros((nrows, 4))
    u0[:nown] = cases.freestream(p)
    # the reference's start-up (transonic-implicit.ctrl): a first-order initialisation solve, then the
    # second-order main solve. Its CFL ramps (25/50 -> 500) blow up on this O-grid's 1e-5 wall cells
    # during the start-up transient (measured), so the main solve's CFL is held fixed
    lin = dict(lin_rtol=1e-2, lin_maxit=lin_maxit, restart=restart, prec_sweeps=sweeps, prec_single=single,
               prec_gs=gs, prec_lines=lines, prec_ilu=ilu, ilu_order=ilu_order, ilu_build_sweeps=ilu_build,
               ilu_apply_sweeps=ilu_apply)
    c0, c1 = init_cfl if init_cfl else (cfl, cfl)
    # the first-order start is timed too: from the free stream its residual falls (on the C4 mesh 2.3e-6
    # -> 3.8e-7 in 5 steps at CFL 25), where the second-order steps that follow are still in the start-up
    # transient (the residual rises for hundreds of steps while the shock forms, profiles/r04/)
    dw = torch.tensor(u0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sp1.steady_backward_euler_device(dw.data_ptr(), fa.ImplicitConfig(cflinit=c0, cflfin=c1, tol=0.0, maxiter=1, **lin))
    del dw                                                       # warm-up: allocations, clocks
    dinit = torch.tensor(u0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if allmax:
        allmax(0.0)
    t0 = time.perf_counter()
    st0, hist0 = sp1.steady_backward_euler_device(dinit.data_ptr(), fa.ImplicitConfig(
        cflinit=c0, cflfin=c1, tol=0.0, maxiter=init_steps, **lin))
    torch.cuda.synchronize()
    dt0 = time.perf_counter() - t0
    if allmax:
        dt0 = allmax(dt0)
    k0 = max(st0["steps"], 1)
    first = {"order": 1, "ms_per_step": round(dt0 / k0 * 1e3, 3), "steps": st0["steps"],
             "lin_iters_per_step": round(st0["lin_iters"] / k0, 2), "resratio": st0["resratio"],
             "res_history": [float(x) for x in hist0], "cfl_ramp": [c0, c1], "final_cfl": st0["cfl"],
             "note": "the first-order start from the free stream (the reference's initialization solve): "
                     "residual + first-order Jacobian + GMRES + update per step, the residual falls"}
    if len(hist0) and hist0[0] == 0.0:
        first["note"] = ("the free stream is a steady state of the first-order density residual here (the initial "
                         "residual is exactly 0, so the start stops after one step and its ratio is 0/0)")
    sp1.close()
    dfree = torch.tensor(u0, dtype=torch.float64, device="cuda")

    def timed(dsrc, mf, var=None):
        du = dsrc.clone()
        torch.cuda.synchronize()  # torch's stream vs the library's (non-blocking) streams
        cfg = fa.ImplicitConfig(cflinit=cfl, cflfin=cfl, tol=0.0, maxiter=warmup, matrix_free=mf, **{**lin, **(var or {})})
        sp.steady_backward_euler_device(du.data_ptr(), cfg)      # warm-up: allocations, clocks
        cfg.maxiter = steps
        dt = 0.0
        for _ in range(max(repeat, 1)):
            du = dsrc.clone()
            torch.cuda.synchronize()
            if allmax:
                allmax(0.0)                                      # a barrier before the timed steps
            t0 = time.perf_counter()
            st, hist = sp.steady_backward_euler_device(du.data_ptr(), cfg)
            torch.cuda.synchronize()
            dt += time.perf_counter() - t0
        dt /= max(repeat, 1)
        if allmax:
            dt = allmax(dt)
        k = max(st["steps"], 1)
        out = {"ms_per_step": round(dt / k * 1e3, 3), "steps": st["steps"],
               "lin_iters_per_step": round(st["lin_iters"] / k, 2),
               "ms_per_lin_iter": round(dt * 1e3 / max(st["lin_iters"], 1), 4),
               "resratio": st["resratio"], "res_history": [float(x) for x in hist]}
        if kernel_times:
            du = dsrc.clone()
            cfg.maxiter = warmup
            torch.cuda.synchronize()
            sp.profile(True)
            sp.steady_backward_euler_device(du.data_ptr(), cfg)
            kt = sp.kernel_times()
            sp.profile(False)
            out["kernel_ms"] = {nm: round(kt[nm][0] / kt[nm][1], 5) for nm in PREC_KERNELS if nm in kt}
            out["kernel_launches"] = {nm: kt[nm][1] for nm in PREC_KERNELS if nm in kt}
        return out

    depths = {}
    if variants or ilu_order:
        depths = {"ilu_order": ilu_order, "ilu_build_sweeps": ilu_build, "ilu_apply_sweeps": ilu_apply,
                  "ilu_depth": {str(o): sp.ilu_order(o)[1] for o in (1, 2)}}
    for mf, (vname, var) in ((mf, v) for mf in operators for v in (variants or [(None, None)])):
        try:
            main_ = timed(dinit if second_from == "start" else dfree, mf, var)
        except RuntimeError as e:
            if vname is None or "diverged" not in str(e):
                raise
            main_ = {"diverged": str(e)}
        if vname is not None:
            main_ = {"variant": vname, "prec": var, **main_}
        out = {"metric": "implicit_step_time", "case": case, "operator": "matrix-free" if mf else "assembled",
               **main_, **depths,
               "cells": mesh.nelem, "faces": mesh.naface, "ranks": world,
               "restart": restart, "prec_sweeps": sweeps, "prec_single": single, "prec_gs": gs, "prec_lines": lines,
               "prec_ilu": ilu, "cfl": cfl,
               "second_order_from": ("the first-order start's state" if second_from == "start" else
                                     "the free stream (a cold start's first second-order steps)"),
               "init": {"steps": st0["steps"], "resratio": st0["resratio"], "cfl_ramp": [c0, c1],
                        "final_cfl": st0["cfl"]},
               "first_order_start": first}
        if second_from != "start":
            # the same steps continuing from the first-order start's state (the reference's two-stage
            # schedule), where this mesh's start-up transient makes the residual rise
            cont = timed(dinit, mf)
            out["after_first_order_start"] = {k: cont[k] for k in ("ms_per_step", "steps", "lin_iters_per_step",
                                                                   "resratio", "res_history")}
        yield out
    sp.close()


if __name__ == "__main__":
    main()
