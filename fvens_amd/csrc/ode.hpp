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
/// out[v] = sum_e area[e] u[e][v], v = 0..3, fixed reduction order (part: 4*512 doubles of scratch)
void launch_conserved(int n, const double* u, const double* area, double* part, double* out, hipStream_t s);
/// out[0] = min_e x[e], -inf if any is NaN (part: 512 doubles of scratch)
void launch_min(int n, const double* x, double* part, double* out, hipStream_t s);

}
#endif
