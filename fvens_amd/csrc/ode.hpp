/** \file ode.hpp
 * \brief Device explicit time stepping helpers (ode.hip). The reductions take `part`, scratch for their partial
 *   results: 512 doubles per reduced value (reduce.hpp RED_CELL_BLOCKS); the handle's reduction scratch
 *   (fvhip_ctx::ensureReductions) holds that.
 */
#ifndef FVHIP_ODE_HPP
#define FVHIP_ODE_HPP

#include <hip/hip_runtime.h>

namespace fvhip {

/// u[e] += cfl*dtm[e] * 1.0/area[e] * r[e]   (aodesolver.cpp:204-214)
void launch_fe_update(int n, const double* r, const double* dtm, const double* area, double cfl, double* u, hipStream_t s);
/// out = (c0*u + c1*us_in) + (sc/area)*r per owned cell: one Runge-Kutta stage. The SSP-RK driver passes
/// sc = c2*h with r = -r(stage state); the TVD-RK driver passes sc = -(c2*dtmin*cfl), which is
/// us = c0*u + c1*us - (c2*dtmin*cfl/area)*r (TVDRKSolver::solve, aodesolver.cpp:735-744) bit for bit.
/// out may be us_in or u, us_in may be u (a lane touches its own row only)
void launch_rk_stage(int n, double c0, double c1, double sc, const double* area, const double* r, const double* u,
                     const double* us_in, double* out, hipStream_t s);
/// g = r - (area/h)*((a0*u + a1*un) + a2*um) per owned cell, the unsteady residual of a BDF step of size h with
/// r = -r(u), and out[0] = sum_e area[e] sum_v g[e][v]^2 in the fixed reduction order (part: 512 doubles of
/// scratch). um is read only when a2 != 0 and may be null otherwise
void launch_bdf_residual(int n, double a0, double a1, double a2, double h, const double* area, const double* r,
                         const double* u, const double* un, const double* um, double* g, double* part, double* out,
                         hipStream_t s);
/// mdt[e] += s*area[e] and the same product added to the four diagonal entries of diag[e] (4x4 blocks): the
/// physical-time term s = a0/h of a BDF step, after the pseudo-time term
void launch_bdf_time_term(int n, double s, const double* area, double* mdt, double* diag, hipStream_t st);
/// out[v] = sum_e area[e] u[e][v], v = 0..3, fixed reduction order (part: 4*512 doubles of scratch)
void launch_conserved(int n, const double* u, const double* area, double* part, double* out, hipStream_t s);
/// out[0] = min_e x[e], -inf if any is NaN (part: 512 doubles of scratch)
void launch_min(int n, const double* x, double* part, double* out, hipStream_t s);

}
#endif
