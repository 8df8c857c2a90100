/** \file ode.hip
 * \brief Device-resident explicit time stepping: SteadyForwardEulerSolver::solve
 *   (aodesolver.cpp:170-240) with the state, residual and time steps kept in HBM.
 *   Update u += cfl*dtm*(1/area)*r in the reference's operation order (:204-214); the Runge-Kutta stage of
 *   the TVD-RK and SSP-RK drivers (explicit.cpp); the conserved sums and the minimum time step, reduced in a
 *   fixed order (two stages, reduce.hpp). The residual norm of the drivers is krylov.hip's energy norm.
 */
#include "ode.hpp"
#include "reduce.hpp"

namespace fvhip {

__global__ void __launch_bounds__(256) k_fe_update(int n, const double* __restrict__ r, const double* __restrict__ dtm,
                                                   const double* __restrict__ area, double cfl, double* __restrict__ u)
{
	const int e = blockIdx.x*blockDim.x + threadIdx.x;
	if(e >= n) return;
	const double a = cfl*dtm[e] * 1.0/area[e];
	const double4 rr = reinterpret_cast<const double4*>(r)[e];
	double4 uu = reinterpret_cast<double4*>(u)[e];
	uu.x += a*rr.x; uu.y += a*rr.y; uu.z += a*rr.z; uu.w += a*rr.w;
	reinterpret_cast<double4*>(u)[e] = uu;
}

/// one Shu-Osher Runge-Kutta stage, out = (c0*u + c1*us_in) + (sc/area)*r, of both drivers of explicit.cpp:
///  - ssprk: r = -r(stage state) as the residual leaves it and sc = c2*h formed on the host;
///  - tvdrk (TVDRKSolver::solve, aodesolver.cpp:735-744: ustage = c0*u + c1*ustage - c2*dtmin*cfl/area*r): the
///    same kernel with sc = -((c2*dtmin)*cfl). (-sc)/area = -(sc/area), (-t)*r = -(t*r) and a + (-x) = a - x are
///    exact in IEEE-754 and this file is built without contraction, so the stage has the bits of the subtraction
///    as written there (tests/test_ssprk_host.py holds the identity on the host).
/// One lane per owned cell reads and writes its own row only, so out may be us_in (middle stages, tvdrk) or u
/// (ssprk's last stage), and us_in may be u (ssprk's first stage): no __restrict__ on them
__global__ void __launch_bounds__(256) k_rk_stage(int n, double c0, double c1, double sc, const double* __restrict__ area,
                                                  const double* __restrict__ r, const double* u,
                                                  const double* us_in, double* out)
{
	const int e = blockIdx.x*blockDim.x + threadIdx.x;
	if(e >= n) return;
	const double t = sc/area[e];
	const double4 rr = reinterpret_cast<const double4*>(r)[e], uu = reinterpret_cast<const double4*>(u)[e];
	double4 ss = reinterpret_cast<const double4*>(us_in)[e];
	ss.x = (c0*uu.x + c1*ss.x) + t*rr.x;
	ss.y = (c0*uu.y + c1*ss.y) + t*rr.y;
	ss.z = (c0*uu.z + c1*ss.z) + t*rr.z;
	ss.w = (c0*uu.w + c1*ss.w) + t*rr.w;
	reinterpret_cast<double4*>(out)[e] = ss;
}

/// sum over owned cells of area*u for the four conserved variables: the fixed partition of the reductions over
/// cells (RED_CELL_BLOCKS blocks, grid-stride) and the fixed tree, so reproducible and without atomics;
/// part [4][gridDim.x], variable-major
__global__ void __launch_bounds__(256) k_conserved_partial(int n, const double* __restrict__ u, const double* __restrict__ area,
                                                           double* __restrict__ part)
{
	double4 acc = make_double4(0, 0, 0, 0);
	for(int e = blockIdx.x*256 + threadIdx.x; e < n; e += 256*gridDim.x) {
		const double a = area[e];
		const double4 uu = reinterpret_cast<const double4*>(u)[e];
		acc.x += a*uu.x; acc.y += a*uu.y; acc.z += a*uu.z; acc.w += a*uu.w;
	}
	double a4[4] = {acc.x, acc.y, acc.z, acc.w};
	block_sum<4>(a4, part + blockIdx.x, static_cast<int>(gridDim.x));
}

/// minimum over cells (order-free), two stages; a NaN anywhere gives -inf (finite values and +inf
/// otherwise as fmin), so the divergence check fires for it and ncclMin across ranks carries it
__global__ void __launch_bounds__(256) k_min_partial(int n, const double* __restrict__ x, double* __restrict__ part)
{
	double m[1] = {INFINITY};
	for(int e = blockIdx.x*256 + threadIdx.x; e < n; e += 256*gridDim.x) m[0] = nan_min(m[0], x[e]);
	block_reduce<1>(m, part + blockIdx.x, 1, RedNanMin{});
}
__global__ void __launch_bounds__(256) k_min_final(int np, const double* __restrict__ part, double* __restrict__ out)
{
	double m[1] = {INFINITY};
	for(int i = threadIdx.x; i < np; i += 256) m[0] = nan_min(m[0], part[i]);
	block_reduce<1>(m, out, 1, RedNanMin{});
	if(threadIdx.x == 0 && out[0] != out[0]) out[0] = -INFINITY;
}

void launch_rk_stage(int n, double c0, double c1, double sc, const double* area, const double* r, const double* u,
                     const double* us_in, double* out, hipStream_t s)
{
	if(n > 0) k_rk_stage<<<(n + 255)/256, 256, 0, s>>>(n, c0, c1, sc, area, r, u, us_in, out);
}

void launch_conserved(int n, const double* u, const double* area, double* part, double* out, hipStream_t s)
{
	k_conserved_partial<<<RED_CELL_BLOCKS, 256, 0, s>>>(n, u, area, part);
	launch_sum_partials(4, RED_CELL_BLOCKS, part, out, s);
}

void launch_min(int n, const double* x, double* part, double* out, hipStream_t s)
{
	k_min_partial<<<RED_CELL_BLOCKS, 256, 0, s>>>(n, x, part);
	k_min_final<<<1, 256, 0, s>>>(RED_CELL_BLOCKS, part, out);
}

void launch_fe_update(int n, const double* r, const double* dtm, const double* area, double cfl, double* u, hipStream_t s)
{
	if(n > 0) k_fe_update<<<(n + 255)/256, 256, 0, s>>>(n, r, dtm, area, cfl, u);
}

}
