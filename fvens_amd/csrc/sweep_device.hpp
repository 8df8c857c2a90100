/** \file sweep_device.hpp
 * \brief What gradients.hip, sweep.hip and fused.hip share: device helpers (vector loads and stores, the
 *   out-of-line boundary ghost state, the cell limiter, the MUSCL pieces) and the host dispatch over the
 *   flux. Each of the three is compiled into namespace `exact` and into namespace `fast` (FVHIP_NS,
 *   FVHIP_FAST; kernels.hpp); the pipeline they form is described in sweep.hip.
 */
#ifndef FVHIP_SWEEP_DEVICE_HPP
#define FVHIP_SWEEP_DEVICE_HPP

#include "kernels.hpp"
#include "blk4.hpp"      // nblk
#include <type_traits>

#ifndef FVHIP_NS
#define FVHIP_NS exact
#endif

namespace fvhip {
namespace FVHIP_NS {

using namespace gd;

/// XCD-aware block -> chunk mapping: the hardware deals consecutive blocks round-robin over the 8
/// XCDs; chunk p = (b%8)*q + b/8 keeps consecutive (Hilbert-adjacent) chunks on one XCD's L2.
/// Launch 8*q blocks; blocks with p >= nchunk return.
__device__ __forceinline__ int xcd_chunk(int nchunk) {
	const int q = (nchunk + 7) >> 3;
	return (static_cast<int>(blockIdx.x) & 7) * q + (static_cast<int>(blockIdx.x) >> 3);
}
static inline int xcd_blocks(long long nchunk) { return static_cast<int>(8*((nchunk + 7)/8)); }

__device__ __forceinline__ void ld4(const double* p, int i, double* o) {
	const double4 v = reinterpret_cast<const double4*>(p)[i];
	o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void st4(double* p, int i, const double* o) {
	reinterpret_cast<double4*>(p)[i] = make_double4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ void ld8(const double* p, int i, double* o) {
	const double4* q = reinterpret_cast<const double4*>(p) + 2*static_cast<size_t>(i);
	const double4 a = q[0], b = q[1];
	o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void st8(double* p, int i, const double* o) {
	double4* q = reinterpret_cast<double4*>(p) + 2*static_cast<size_t>(i);
	q[0] = make_double4(o[0], o[1], o[2], o[3]); q[1] = make_double4(o[4], o[5], o[6], o[7]);
}

/// Boundary ghost state out of line (abc.cpp via gasdyn.hpp ghost_state): boundary faces are rare
/// (~sqrt(N)), but every BC type inlined into the hot kernels' unrolled neighbour loops costs
/// registers, i.e. occupancy, on every cell and face. Arguments and result travel in registers.
__device__ __noinline__ double4 ghost_ool(const Gas G, const BCDev bc, const double4 uinf, const double4 ins,
                                          const double2 nn)
{
	const double ui[4] = {uinf.x, uinf.y, uinf.z, uinf.w}, in[4] = {ins.x, ins.y, ins.z, ins.w};
	const double n[2] = {nn.x, nn.y};
	double gs[4];
	ghost_state(G, bc, ui, in, n, gs);
	return make_double4(gs[0], gs[1], gs[2], gs[3]);
}
__device__ __forceinline__ void ghost(const DevPhys& P, int bc, const double* ins, const double* n, double* gs)
{
	const double4 g = ghost_ool(P.gas, P.bc[bc], make_double4(P.uinf[0], P.uinf[1], P.uinf[2], P.uinf[3]),
	                            make_double4(ins[0], ins[1], ins[2], ins[3]), make_double2(n[0], n[1]));
	gs[0] = g.x; gs[1] = g.y; gs[2] = g.z; gs[3] = g.w;
}

/// an empty register constraint: the value must exist in VGPRs here, so a load producing it cannot be
/// merged with another load behind a pointer select
__device__ __forceinline__ void pin_regs(double& x) { asm("" : "+v"(x)); }

/// limiter values of one cell (k_limiter's arithmetic): uc its primitive state, g its gradient,
/// un[j] / gp[j] the state across and the centre of its face j (any face order: dmin/dmax and the
/// minimum over faces do not depend on it), nf faces.
/// Venkatakrishnan (limitedlinearreconstruction.cpp:219-246) in fewer instructions, bitwise: 2*dp*dm
/// and 2*dm*dm scale exact products (2 RN(dp dm), 2 RN(dm dm)), so each sum that adds one is an fma with
/// the factor 2, and dp*dm is formed once for numerator and denominator; the running max / min are
/// v_max / v_min -- they differ from the reference's compare-and-assign only in the sign of a zero
/// dmin/dmax (max(+0, -0)), and a signed zero dp gives the same phi (dp*dp = +0, +0 + (+-0) = +0).
/// (A one-division-per-variable variant -- exact arg-min by cross-multiplication, only the winner divided --
/// was bitwise but 1.2-1.7 % slower: DESIGN.md section 8, profiles/r05/venk_onediv_ab.txt.)
template <bool VENK>
__device__ __forceinline__ void cell_limiter(const double* uc, const double* g, const double (*un)[4],
                                             const double2* gp, const bool* has, double2 r, double eps2,
                                             double* out)
{
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) {
		double dmin = 0, dmax = 0;
		#pragma unroll
		for(int j = 0; j < 4; j++) {
			if(!has[j]) continue;
			const double d = un[j][iv]-uc[iv];
			if(VENK) { dmax = __builtin_fmax(dmax, d); dmin = __builtin_fmin(dmin, d); }
			else {
				if(d > dmax) dmax = d;
				if(d < dmin) dmin = d;
			}
		}
		double lim = 1.0;
		#pragma unroll
		for(int j = 0; j < 4; j++) {
			if(!has[j]) continue;
			double uf = uc[iv];
			uf += 1.0*g[iv*2+0]*(gp[j].x - r.x);
			uf += 1.0*g[iv*2+1]*(gp[j].y - r.y);
			double ph;
			if(VENK) {
				const double dm = uf - uc[iv];
				const double dp = dm < 0 ? dmin : dmax;
				const double pp = dp*dp, pm = dp*dm;
				// (dp*dp + 2*dp*dm + eps2)/(dp*dp + dp*dm + 2*dm*dm + eps2)
				const double n = __builtin_fma(pm, 2.0, pp) + eps2, d = __builtin_fma(dm*dm, 2.0, pp + pm) + eps2;
				lim = __builtin_fmin(lim, div_rn(n, d));
				continue;
			} else {
				const double diff = uf - uc[iv];
				if(diff > 0) ph = 1 < dmax/diff ? 1 : dmax/diff;
				else if(diff < 0) ph = 1 < dmin/diff ? 1 : dmin/diff;
				else ph = 1;
			}
			if(ph < lim) lim = ph;
		}
		out[iv] = lim;
	}
}

/// MUSCL / Van Albada pieces (musclreconstruction.cpp:33-59, 86-90, 112-120), bitwise in fewer
/// instructions: the numerator 2.0*d*du + eps as fma(d*du, 2, eps) (2d is exact, so RN(2d*du) =
/// 2 RN(d*du)); `phi < 0 -> 0` as one v_max (phi is never -0: the numerator RN(x + 1e-8) is +0 when
/// x = -1e-8, and the denominator is positive); ui + phi/4.0*S as fma(phi*S, 1/4, ui) (add_pow2)
__device__ __forceinline__ double muscl_phi(double d, double du) {
	const double eps = 1e-8;
	const double ph = div_rn(__builtin_fma(d*du, 2.0, eps), d*d + du*du + eps);
	return __builtin_fmax(ph, 0.0);
}
__device__ __forceinline__ double muscl_left(double ui, double uj, double dm, double ph) {
	const double k = 1.0/3.0;
	return add_pow2(ui, ph*( (1.0-k*ph)*dm + (1.0+k*ph)*(uj - ui) ), 0.25);
}
__device__ __forceinline__ double muscl_right(double ui, double uj, double dp, double ph) {
	const double k = 1.0/3.0;
	return add_pow2(uj, ph*( (1.0-k*ph)*dp + (1.0+k*ph)*(uj - ui) ), -0.25);
}

// (The loops that use these pieces -- MUSCL interior face, MUSCL boundary face, linear extrapolation -- are
// spelt out in k_sweep and again in the fused residual's fz_body, and must stay equal: as __forceinline__
// helpers here they changed the machine code of every second-order instantiation of both kernels,
// profiles/kernels_split/SOURCES.md.)

// ------------------------------------------------------------------------------------------------
// host dispatch over the flux (k_sweep, k_residual_wls)
// ------------------------------------------------------------------------------------------------
/// f(std::integral_constant<int, FLUX>) for the run-time flux; out of range: HLLC (6), as flux_index
template <typename F>
static inline auto with_flux(int flux, F&& f)
{
	switch(flux) {
		case 0: return f(std::integral_constant<int, 0>());
		case 1: return f(std::integral_constant<int, 1>());
		case 2: return f(std::integral_constant<int, 2>());
		case 3: return f(std::integral_constant<int, 3>());
		case 4: return f(std::integral_constant<int, 4>());
		case 5: return f(std::integral_constant<int, 5>());
		default: return f(std::integral_constant<int, 6>());
	}
}
static inline int flux_index(int flux) { return flux < 0 || flux > 6 ? 6 : flux; }

/// the names a kernel family reports for profiling, by flux: "k_sweep<ROE>", in namespace fast "k_sweep_fast<ROE>"
#ifdef FVHIP_FAST
#define FVHIP_KSUFFIX "_fast"
#else
#define FVHIP_KSUFFIX ""
#endif
#define FVHIP_FLUX_NAMES(k) { k FVHIP_KSUFFIX "<LLF>", k FVHIP_KSUFFIX "<VANLEER>", k FVHIP_KSUFFIX "<AUSM>", \
	k FVHIP_KSUFFIX "<AUSMPLUS>", k FVHIP_KSUFFIX "<ROE>", k FVHIP_KSUFFIX "<HLL>", k FVHIP_KSUFFIX "<HLLC>" }

}
}
#endif
