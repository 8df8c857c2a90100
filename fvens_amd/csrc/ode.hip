/** \file ode.hip
 * \brief Device-resident explicit time stepping: SteadyForwardEulerSolver::solve
 *   (aodesolver.cpp:170-240) with the state, residual and time steps kept in HBM.
 *   Update u += cfl*dtm*(1/area)*r in the reference's operation order (:204-214); the Runge-Kutta stage of
 *   the TVD-RK and SSP-RK drivers (explicit.cpp); the unsteady residual and the physical-time term of the BDF
 *   dual-time driver (implicit.cpp); the conserved sums and the minimum time step, reduced in a
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

/// the unsteady residual of a BDF step of size h (implicit.cpp dualTime),
///   G = r - (area/h)*((a0*u + a1*un) + a2*um),   r = -r(u) as the residual leaves it,
/// in that association with area/h formed once per cell, and in the same pass the block partials of
/// sum_c area_c sum_v G_cv^2 (the energy norm's weighting over all four variables) in the fixed partition of the
/// reductions over cells. um is read only when a2 != 0 (BDF1 and the first step of BDF2 pass null): the branch is
/// on a kernel argument, so uniform. 136 B read (104 B without um) and 32 B written per cell
__global__ void __launch_bounds__(256) k_bdf_residual(int n, double a0, double a1, double a2, double h,
                                                      const double* __restrict__ area, const double* __restrict__ r,
                                                      const double* __restrict__ u, const double* __restrict__ un,
                                                      const double* __restrict__ um, double* __restrict__ g,
                                                      double* __restrict__ part)
{
	double acc[1] = {0.0};
	for(int e = blockIdx.x*256 + threadIdx.x; e < n; e += 256*gridDim.x) {
		const double a = area[e], q = a/h;
		const double4 rr = reinterpret_cast<const double4*>(r)[e], uu = reinterpret_cast<const double4*>(u)[e];
		const double4 nn = reinterpret_cast<const double4*>(un)[e];
		double4 d = make_double4(a0*uu.x + a1*nn.x, a0*uu.y + a1*nn.y, a0*uu.z + a1*nn.z, a0*uu.w + a1*nn.w);
		if(a2 != 0.0) {
			const double4 mm = reinterpret_cast<const double4*>(um)[e];
			d.x += a2*mm.x; d.y += a2*mm.y; d.z += a2*mm.z; d.w += a2*mm.w;
		}
		const double4 gg = make_double4(rr.x - q*d.x, rr.y - q*d.y, rr.z - q*d.z, rr.w - q*d.w);
		reinterpret_cast<double4*>(g)[e] = gg;
		acc[0] += a*(((gg.x*gg.x + gg.y*gg.y) + gg.z*gg.z) + gg.w*gg.w);
	}
	block_sum<1>(acc, part + blockIdx.x, 1);
}

/// the physical-time term of a BDF step on top of the pseudo-time term (k_jac_diag / k_pseudo_time have left
/// m = area/(cfl dtm) in mdt and added it to the diagonal): mdt[c] += s*area[c] and the same product added to
/// the four diagonal entries of the cell's block, s = a0/h. Four lanes per cell, lane i holds row i of the block
/// (one 32-byte row read and written back; the twelve other entries keep their bits)
__global__ void __launch_bounds__(256) k_bdf_time_term(int n, double s, const double* __restrict__ area,
                                                       double* __restrict__ mdt, double* __restrict__ diag)
{
	const long long t = blockIdx.x*256LL + threadIdx.x;
	if(t >= 4LL*n) return;
	const int c = static_cast<int>(t >> 2), i = static_cast<int>(t & 3);
	const double p = s*area[c];
	double4 row = reinterpret_cast<double4*>(diag)[t];
	if(i == 0) { row.x += p; mdt[c] += p; }
	else if(i == 1) row.y += p;
	else if(i == 2) row.z += p;
	else row.w += p;
	reinterpret_cast<double4*>(diag)[t] = row;
}

void launch_bdf_residual(int n, double a0, double a1, double a2, double h, const double* area, const double* r,
                         const double* u, const double* un, const double* um, double* g, double* part, double* out,
                         hipStream_t s)
{
	k_bdf_residual<<<RED_CELL_BLOCKS, 256, 0, s>>>(n, a0, a1, a2, h, area, r, u, un, um, g, part);
	launch_sum_partials(1, RED_CELL_BLOCKS, part, out, s);
}

void launch_bdf_time_term(int n, double s, const double* area, double* mdt, double* diag, hipStream_t st)
{
	if(n > 0) k_bdf_time_term<<<static_cast<unsigned>((4LL*n + 255)/256), 256, 0, st>>>(n, s, area, mdt, diag);
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
