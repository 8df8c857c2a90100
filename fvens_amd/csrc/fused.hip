/** \file fused.hip
 * \brief The one-launch fused residual of the MI355X face sweep (gfx950, wave64): k_residual_wls, its
 *   probe build and its dispatch. The pipeline it fuses is described in sweep.hip.
 */
#include "sweep_device.hpp"
#include <algorithm>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>

namespace fvhip {
namespace FVHIP_NS {

// ------------------------------------------------------------------------------------------------
// THE FUSED RESIDUAL (WLS gradients + MUSCL / unlimited linear reconstruction, inviscid)
// One launch per residual: every patch stages its cells and its ring-1 cells (far side of its cut
// faces) in LDS as primitive states, recomputes their WLS gradients there (ring-2 neighbours come
// from global memory), then sweeps its faces and sums them per cell. Same operations, same order as
// k_prep_grad_wls + k_sweep: the result is bitwise the staged path's. Ring-1 gradients are computed
// by every patch that needs them (35 % more gradients on C4) instead of a round trip through HBM.
// LDS row per staged cell (14 doubles): [up 4][gradient 8][rc 2]; viscous instantiations 18:
// [up 4][gradient 8][rc 2][T, dT/dx, dT/dy, pad] (the temperature terms of fz_viscous, per gradient row)
// ------------------------------------------------------------------------------------------------
constexpr int FZW = 14;
constexpr int FZW_VISC = 18;
template <int VISC> constexpr int fz_w() { return VISC != SV_NONE ? FZW_VISC : FZW; }

/// primitive ghost state of a cell's value across boundary face bf (k_prep_bfaces arithmetic)
/// the fused residual's ghost states: the common BC types' ghost_state (gasdyn.hpp ghost_state_common)
/// inlined -- fusedEligible admits only configurations whose BCs are all of those types (the others
/// take the staged path). An out-of-line call in this kernel (ghost_ool: 82 VGPRs of its own, and the
/// caller's values kept live across the call) costs 28 VGPRs on every path: 118 instead of 90 for the
/// inviscid kernel, i.e. 4 instead of 5 waves per SIMD; 162 instead of 124 for the limited ones
__device__ __forceinline__ void ghost_c(const DevPhys& P, int bc, const double* ins, const double* n, double* gs)
{
	const double ui[4] = {P.uinf[0], P.uinf[1], P.uinf[2], P.uinf[3]};
	ghost_state_common(P.gas, P.bc[bc], ui, ins, n, gs);
}
/// the conserved state row of cell c the fused residual works on: u[c], or with the fused matrix-free
/// operator (SweepBuffers::mfx; MF: instantiations without time steps only) the perturbed state
/// u[c] + pm[1] x[c], k_mf_perturb's arithmetic
template <bool MF>
__device__ __forceinline__ void ld_state(const SweepBuffers& B, int c, double* o)
{
	ld4(B.u, c, o);
	if(MF && B.mfx) {
		double x[4];
		ld4(B.mfx, c, x);
		const double s = B.mfpm[1];
		#pragma unroll
		for(int i = 0; i < 4; i++) o[i] = o[i] + s*x[i];
	}
}
template <bool MF>
__device__ __forceinline__ double4 ghost_prim_of_cell(const DevMesh& M, const DevPhys& P, const SweepBuffers& B, int cell, int bf)
{
	const double2 nn = M.bf_n[bf];
	const double n[2] = {nn.x, nn.y};
	double ucons[4], gs[4], gp[4];
	ld_state<MF>(B, cell, ucons);
	ghost_c(P, M.bf_bc[bf], ucons, n, gs);
	cons2prim(P.gas, gs, gp);
	return make_double4(gp[0], gp[1], gp[2], gp[3]);
}

/// phase 0 of the fused residual: a staged row [up 4][gradient 8][rc 2] from the conserved state
__device__ __forceinline__ void stage_row(const Gas& G, double* row, const double* ucons, double2 r)
{
	double b[4];
	cons2prim(G, ucons, b);
	st4(row, 0, b);
	*reinterpret_cast<double2*>(row + 12) = r;
}

/// The fused residual rebuilds each cell's WLS inverse from the staged centres it already reads instead of
/// loading the precomputed one (32 B per gradient row less traffic).
/// One neighbour's term of the WLS normal matrix, V[2i+j] += w2*dr[i]*dr[j] (agradientschemes.cpp:
/// 218-317 as restated in layout.cpp: w2*dr[i] first, then times dr[j])
__device__ __forceinline__ void wls_normal_add(double* vm, double w2, double d0, double d1)
{
	const double a = w2*d0, b = w2*d1;
	vm[0] += a*d0; vm[1] += a*d1; vm[2] += b*d0; vm[3] += b*d1;
}
/// the first neighbour's term, 0 + w2*dr[i]*dr[j] (mul0)
__device__ __forceinline__ void wls_normal_first(double* vm, double w2, double d0, double d1)
{
	const double a = w2*d0, b = w2*d1;
	vm[0] = mul0(a, d0); vm[1] = mul0(a, d1); vm[2] = mul0(b, d0); vm[3] = mul0(b, d1);
}
/// its inverse, the host's 2x2 inverse arithmetic (layout.cpp, Eigen's inverse for 2x2)
__device__ __forceinline__ double4 wls_inverse(const double* v)
{
	const double det = v[0]*v[3] - v[2]*v[1];
	const double invdet = div_rn(1.0, det);
	return make_double4(v[3]*invdet, -v[1]*invdet, -v[2]*invdet, v[0]*invdet);
}

/// phase 1 of the fused residual: WLS gradient of staged row `row` (cell c) from the staged rows of
/// its neighbours nb4 (patch-local indices, boundary codes -2-bf, -1 padding), k_prep_grad_wls
/// arithmetic; a ghost cell takes the gradient received from its owner
/// the centres of cell c's faces in ascending reference face order (k_prep_grad_wls<LIM>'s source:
/// cell_slots -> slot_gr); padding entries (0, 0)
__device__ __forceinline__ void fz_face_centres(const DevMesh& M, int c, double2* gp)
{
	const int4 cs = M.cell_slots[c];
	const int sl[4] = {cs.x, cs.y, cs.z, cs.w};
	#pragma unroll
	for(int k = 0; k < 4; k++) gp[k] = sl[k] >= 0 ? M.slot_gr[sl[k] >> 1] : make_double2(0, 0);
}
template <int LIM, int W = FZW, bool MF = false>
__device__ __forceinline__ void fused_limit_row(const DevMesh& M, const DevPhys& P, const SweepBuffers& B,
                                                const double* fz, const double* row, int c, int4 nb4,
                                                const double2* gp, double eps2, double* g);
/// viscous rows (W = FZW_VISC): the temperature and its gradient of the row's cell, the arithmetic
/// fz_viscous applied per face side until round 4 (temperature(rho, p), grad_temperature per direction
/// from the density and pressure gradients), formed once per gradient row instead
template <int W>
__device__ __forceinline__ void fz_row_temperature(const Gas& G, double* row, const double* g)
{
	if constexpr(W == FZW_VISC) {
		const double rho = row[0], p = row[3];
		const double tx = grad_temperature(G, rho, g[0*2+0], p, g[3*2+0]);
		const double ty = grad_temperature(G, rho, g[0*2+1], p, g[3*2+1]);
		*reinterpret_cast<double2*>(row + 14) = make_double2(temperature(G, rho, p), tx);
		row[16] = ty;
	}
}
template <int LIM, int W = FZW, bool MF = false>
__device__ __forceinline__ void fused_wls_row(const DevMesh& M, const DevPhys& P, const SweepBuffers& B,
                                              const double* fz, double* row, int c, int4 nb4,
                                              const double2* gp = nullptr, double eps2 = 0.0)
{
	static_assert(!(LIM && W == FZW_VISC), "limited reconstructions are not fused with the viscous flux");
	if(c >= M.nown) {
		double g[8];
		ld8(B.grad, c, g);
		if(LIM) {
			// layer-1 ghost of a two-layer halo: its limiter values were computed locally
			// (k_grad_ghost<LIM>); lim*g as fused_limit_row forms it
			double lim[4];
			ld4(B.phi, c, lim);
			#pragma unroll
			for(int iv = 0; iv < 4; iv++) { g[iv*2+0] = lim[iv]*g[iv*2+0]; g[iv*2+1] = lim[iv]*g[iv*2+1]; }
		}
		st8(row + 4, 0, g);
		fz_row_temperature<W>(P.gas, row, g);
		return;
	}
	double uc[4];
	ld4(row, 0, uc);
	const double2 rcc = *reinterpret_cast<const double2*>(row + 12);
	double f[8] = {0,0,0,0,0,0,0,0};
	double vm[4] = {0, 0, 0, 0};     // WLS normal matrix, same terms and order as the host's
	if(nb4.x >= 0 && nb4.y >= 0 && nb4.z >= 0 && nb4.w >= -1) {
		// no boundary neighbour (all but ~0.1 % of the rows): every neighbour is an LDS row. The
		// first three (every triangle and quad has them) are requested at once and their weights
		// computed side by side instead of one LDS round trip and one division chain after another;
		// the fourth (quads) follows
		const int nb[3] = {nb4.x, nb4.y, nb4.z};
		double w[3], d0[3], d1[3], un[3][4];
		#pragma unroll
		for(int k = 0; k < 3; k++) {
			const double* nrow = &fz[nb[k]*W];
			const double2 rn = *reinterpret_cast<const double2*>(nrow + 12);
			ld4(nrow, 0, un[k]);
			double w2 = mul0(rcc.x-rn.x, rcc.x-rn.x);
			w2 += (rcc.y-rn.y)*(rcc.y-rn.y);
			d0[k] = rcc.x-rn.x; d1[k] = rcc.y-rn.y;
			w[k] = div_rn(1.0, w2);
		}
		// the sums start from zero: the first neighbour's terms are 0 + a*b (mul0)
		#pragma unroll
		for(int iv = 0; iv < 4; iv++) {
			const double du = uc[iv] - un[0][iv];
			f[iv*2+0] = mul0(w[0]*d0[0], du);
			f[iv*2+1] = mul0(w[0]*d1[0], du);
		}
		wls_normal_first(vm, w[0], d0[0], d1[0]);
		#pragma unroll
		for(int k = 1; k < 3; k++) {
			#pragma unroll
			for(int iv = 0; iv < 4; iv++) {
				const double du = uc[iv] - un[k][iv];
				f[iv*2+0] += w[k]*d0[k]*du;
				f[iv*2+1] += w[k]*d1[k]*du;
			}
			wls_normal_add(vm, w[k], d0[k], d1[k]);
		}
		if(nb4.w >= 0) {
			const double* nrow = &fz[nb4.w*W];
			const double2 rn = *reinterpret_cast<const double2*>(nrow + 12);
			double u3[4];
			ld4(nrow, 0, u3);
			double w2 = mul0(rcc.x-rn.x, rcc.x-rn.x);
			w2 += (rcc.y-rn.y)*(rcc.y-rn.y);
			const double e0 = rcc.x-rn.x, e1 = rcc.y-rn.y;
			w2 = div_rn(1.0, w2);
			#pragma unroll
			for(int iv = 0; iv < 4; iv++) {
				const double du = uc[iv] - u3[iv];
				f[iv*2+0] += w2*e0*du;
				f[iv*2+1] += w2*e1*du;
			}
			wls_normal_add(vm, w2, e0, e1);
		}
	} else
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		const int nbk = k == 0 ? nb4.x : (k == 1 ? nb4.y : (k == 2 ? nb4.z : nb4.w));
		if(nbk == -1) break;
		// the LDS row is read unconditionally (row 0 for a boundary code) and pinned in registers
		// before the boundary values may replace it: otherwise the compiler merges the two loads
		// into one generic (flat) load of a selected pointer, which waits on every outstanding
		// global load of the wave
		double un[4];
		const double* nrow = &fz[(nbk >= 0 ? nbk : 0)*W];
		ld4(nrow, 0, un);
		double2 rn = *reinterpret_cast<const double2*>(nrow + 12);
		pin_regs(un[0]); pin_regs(un[1]); pin_regs(un[2]); pin_regs(un[3]); pin_regs(rn.x); pin_regs(rn.y);
		if(nbk < 0) {
			const int bf = -2 - nbk;
			const double4 gp = ghost_prim_of_cell<MF>(M, P, B, c, bf);
			un[0] = gp.x; un[1] = gp.y; un[2] = gp.z; un[3] = gp.w;
			rn = M.bf_rcbp[bf];
		}
		double w2 = 0;
		w2 += (rcc.x-rn.x)*(rcc.x-rn.x);
		w2 += (rcc.y-rn.y)*(rcc.y-rn.y);
		const double dr0 = rcc.x-rn.x, dr1 = rcc.y-rn.y;
		w2 = div_rn(1.0, w2);
		#pragma unroll
		for(int iv = 0; iv < 4; iv++) {
			const double du = uc[iv] - un[iv];
			f[iv*2+0] += w2*dr0*du;
			f[iv*2+1] += w2*dr1*du;
		}
		wls_normal_add(vm, w2, dr0, dr1);
	}
	const double4 V = wls_inverse(vm);
	double g[8];
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) {
		g[iv*2+0] = V.x*f[iv*2+0] + V.y*f[iv*2+1];
		g[iv*2+1] = V.z*f[iv*2+0] + V.w*f[iv*2+1];
	}
	if(LIM) fused_limit_row<LIM, W, MF>(M, P, B, fz, row, c, nb4, gp, eps2, g);
	st8(row + 4, 0, g);
	fz_row_temperature<W>(P.gas, row, g);
}

/// limited reconstructions in the fused residual: the row's Barth-Jespersen / Venkatakrishnan limiter
/// values from the staged neighbour states (boundary: the ghost primitive state, as the staged path)
/// and its face centres, k_prep_grad_wls<LIM>'s arithmetic; the staged row then holds lim*g, which is
/// the product linearExtrapolate forms first ((lim*grad)*(gp - rc), reconstruction_utils.hpp:28-30)
template <int LIM, int W, bool MF>
__device__ __forceinline__ void fused_limit_row(const DevMesh& M, const DevPhys& P, const SweepBuffers& B,
                                                const double* fz, const double* row, int c, int4 nb4,
                                                const double2* gpre, double eps2, double* g)
{
	double uc[4];
	ld4(row, 0, uc);
	const double2 rcc = *reinterpret_cast<const double2*>(row + 12);
	double2 gp[4];
	if(gpre) { gp[0] = gpre[0]; gp[1] = gpre[1]; gp[2] = gpre[2]; gp[3] = gpre[3]; }
	else { fz_face_centres(M, c, gp); eps2 = LIM == 2 ? M.venk_eps2[c] : 0.0; }
	const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
	double un[4][4];
	bool has[4];
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		has[k] = nb[k] != -1;
		un[k][0] = un[k][1] = un[k][2] = un[k][3] = 0.0;
		if(!has[k]) continue;
		if(nb[k] >= 0) ld4(&fz[nb[k]*W], 0, un[k]);
		else {
			const double4 q = ghost_prim_of_cell<MF>(M, P, B, c, -2 - nb[k]);
			un[k][0] = q.x; un[k][1] = q.y; un[k][2] = q.z; un[k][3] = q.w;
		}
	}
	double lim[4];
	cell_limiter<LIM == 2>(uc, g, un, gp, has, rcc, eps2, lim);
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) { g[iv*2+0] = lim[iv]*g[iv*2+0]; g[iv*2+1] = lim[iv]*g[iv*2+1]; }
}

/// the modified-average viscous flux of one face in the fused residual (gasdyn.hpp viscous_flux_core's
/// arithmetic, same operations in the same order, so bitwise its result), streamed from the staged LDS
/// rows variable by variable: first the temperature terms (density and pressure values and gradients),
/// then the velocity terms, each group read after a compiler fence, so only one group's LDS values are
/// live at a time instead of both cells' full rows (24 doubles) -- register pressure. The density
/// face gradient (unused by the flux) is not formed. Boundary face: rowj = nullptr, the right state is
/// the ghost primitive state gpr and the right gradient the cell's own.
__device__ __forceinline__ void fz_viscous(const Gas& G, const double* rowi, const double* rowj, const double4 gpr,
                                           double4 vg, const double* n, double muRe, const double* va, double* vf)
{
	const double* gsrc = rowj ? rowj : rowi;          // right gradient: the boundary cell's own
	// the face's unit vector between the centres (vg: left xy, right xy) and their distance (0 + dx^2 + dy^2,
	// correctly rounded root and quotients; reading them per slot from HBM was slower)
	double dr[2], dist = 0;
	dr[0] = vg.z - vg.x; dist += dr[0]*dr[0];
	dr[1] = vg.w - vg.y; dist += dr[1]*dr[1];
	dist = sqrt_rn(dist);
	dr[0] = div_rn(dr[0], dist); dr[1] = div_rn(dr[1], dist);
	double grad[2][4];
	{   // temperature: T and dT of each side, formed per staged row in phase 1 (fz_row_temperature); a
		// boundary face's right side is the ghost state with the cell's own gradients, formed here
		__asm__ volatile("" ::: "memory");
		const double2 tgl = *reinterpret_cast<const double2*>(rowi + 14);
		const double gL[2] = {tgl.y, rowi[16]}, tl = tgl.x;
		double gR[2], tr;
		if(rowj) {
			const double2 tgr = *reinterpret_cast<const double2*>(rowj + 14);
			gR[0] = tgr.y; gR[1] = rowj[16]; tr = tgr.x;
		} else {
			const double rrr = gpr.x, prr = gpr.w;
			for(int j = 0; j < 2; j++) gR[j] = grad_temperature(G, rrr, gsrc[4 + 0*2 + j], prr, gsrc[4 + 3*2 + j]);
			tr = temperature(G, rrr, prr);
		}
		double davg[2];
		davg[0] = 0.5*(gL[0] + gR[0]);
		davg[1] = 0.5*(gL[1] + gR[1]);
		const double corr = div_rn(tr-tl, dist);
		const double ddr = dot2(davg,dr);
		grad[0][3] = davg[0] - ddr*dr[0] + corr*dr[0];
		grad[1][3] = davg[1] - ddr*dr[1] + corr*dr[1];
	}
	#pragma unroll
	for(int i = 1; i < 3; i++) {   // velocity components
		__asm__ volatile("" ::: "memory");
		const double tl = rowi[i], tr = rowj ? rowj[i] : (i == 1 ? gpr.y : gpr.z);
		double davg[2];
		davg[0] = 0.5*(rowi[4 + i*2 + 0] + gsrc[4 + i*2 + 0]);
		davg[1] = 0.5*(rowi[4 + i*2 + 1] + gsrc[4 + i*2 + 1]);
		const double corr = div_rn(tr-tl, dist);
		const double ddr = dot2(davg,dr);
		grad[0][i] = davg[0] - ddr*dr[0] + corr*dr[0];
		grad[1][i] = davg[1] - ddr*dr[1] + corr*dr[1];
	}
	const double kd = div_rcp(muRe, G.kden, G.rkden);
	double ldiv = 0;
	ldiv += grad[0][1]; ldiv += grad[1][2];
	ldiv *= 2.0/3.0*muRe;
	// s[i][i] = muRe*(g + g) - ldiv: muRe*(2g) = 2 RN(muRe g) exactly, so one fma with the factor 2
	double s[2][2];
	s[0][0] = __builtin_fma(muRe*grad[0][1], 2.0, -ldiv); s[0][1] = muRe*(grad[0][2] + grad[1][1]);
	s[1][0] = muRe*(grad[1][1] + grad[0][2]); s[1][1] = __builtin_fma(muRe*grad[1][2], 2.0, -ldiv);
	vf[0] = 0;
	for(int i = 0; i < 2; i++) { double t = 0; t -= s[i][0]*n[0]; t -= s[i][1]*n[1]; vf[i+1] = t; }
	double e = 0;
	for(int i = 0; i < 2; i++) {
		double comp = 0;
		comp += s[i][0]*va[0]; comp += s[i][1]*va[1];
		comp += kd*grad[i][3];
		e -= comp * n[i];
	}
	vf[3] = e;
}

// Probe build (make EXTRA=-DFVHIP_FZ_STAMPS, into an OBJDIR and LIB of its own; tools/fz_stamps.py):
// every wave reads the shader clock at seven points of k_residual_wls and thread 0 of each block writes
// them at the end, with the wall-clock ticks from the first to the last, to SweepBuffers::stamps
// (eight 64-bit words per block). The stamps stay in scalar registers until then, so no store joins
// the loads the kernel waits for. Without the define nothing of this is compiled.
#ifdef FVHIP_FZ_STAMPS
struct FzStamps { unsigned long long t[7], w0; };
#define FZ_STAMPS_PARAM , FzStamps& stamps
#define FZ_STAMPS_ARG , stamps
/// a stamp that what the program has issued so far in source order precedes
#define FZ_STAMP(k) do { asm volatile("" ::: "memory"); stamps.t[k] = __builtin_amdgcn_s_memtime(); \
                         asm volatile("" ::: "memory"); } while(0)
/// The two stamps ahead of the patch metadata read the clock in an asm statement that is not volatile and
/// is ordered by its inputs alone: anything with side effects there (the clock builtin included) makes the
/// compiler load the metadata with vector instead of scalar loads, i.e. measure another kernel. The
/// entry stamp takes the block index, the other the (uniform) values a, b, c, d it is to follow.
#define FZ_STAMP_ENTRY() asm("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamps.t[0]) : "s"(blockIdx.x))
#define FZ_STAMP_AFTER(k, a, b, c, d) asm("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamps.t[k]) \
                                          : "s"(a), "s"(b), "s"(c), "s"(d))
#else
#define FZ_STAMPS_PARAM
#define FZ_STAMPS_ARG
#define FZ_STAMP(k) do {} while(0)
#define FZ_STAMP_ENTRY() do {} while(0)
#define FZ_STAMP_AFTER(k, a, b, c, d) do {} while(0)
#endif

/// one patch of the fused residual: uniform (scalar) metadata
struct FzPatch { int p, s0, s1, c0, c1, nc, e0, nl, ng; const uint2* gnbr; const int* gbf; };
/// what one thread loads for its patch before phase 0: its first staged row (state, centre), the
/// neighbour list and WLS inverse of the gradient it computes first, and the geometry of its face
struct FzPre { int cf; double ua[4]; double2 rca; int4 nb4a; int2 lrl; double2 nn; double len;
               double2 gpa[4]; double eps2a; };     // gpa, eps2a: limited reconstructions' first-row inputs

/// the patch's record (layout.hpp FzPatchRec): one uniform 32-byte load instead of three dependent
/// rounds of scalar loads from six arrays
__device__ __forceinline__ FzPatch fz_patch(const DevMesh& M, const SweepBuffers& B, int pi)
{
	FzPatch q;
	q.p = B.plist ? B.plist[pi] : pi;
	const FzPatchMeta m = fz_unpack(M.fz_rec[q.p]);
	q.s0 = m.s0; q.s1 = m.s0 + m.ns;
	q.c0 = m.c0; q.c1 = m.c0 + m.nc;
	q.nc = m.nc;
	q.e0 = m.e0;
	q.nl = m.nl;                                      // staged rows: patch, ring 1, ring 2
	q.ng = m.ng;                                      // rows whose gradients the patch computes
	q.gnbr = M.fz_gnbr16 + m.g0;
	q.gbf = M.fz_gbf + m.gbf0;
	return q;
}
/// a gradient row's four packed neighbour codes (layout.hpp fz_gnbr16) as patch-local index,
/// -2-bf (boundary face) or -1 (none)
__device__ __forceinline__ int fz_nbr_code(unsigned x, const int* gbf)
{
	if(x == 0xFFFFu) return -1;
	if(x & 0x8000u) return -2 - gbf[x & 0x7FFFu];
	return static_cast<int>(x);
}
__device__ __forceinline__ int4 fz_nbr_codes(uint2 v, const int* gbf)
{
	return make_int4(fz_nbr_code(v.x & 0xFFFFu, gbf), fz_nbr_code(v.x >> 16, gbf),
	                 fz_nbr_code(v.y & 0xFFFFu, gbf), fz_nbr_code(v.y >> 16, gbf));
}
__device__ __forceinline__ int4 fz_nbrs(const FzPatch& q, int i) { return fz_nbr_codes(q.gnbr[i], q.gbf); }
__device__ __forceinline__ int fz_cell(const DevMesh& M, const FzPatch& q, int i)
{
	return i < q.nc ? q.c0 + i : M.fz_ext[q.e0 + (i - q.nc)];
}
/// The loads of FzPre, ordered by what they depend on. Everything here needs only the patch record, except
/// the ring rows' state and centre, which need the ring cell id: that id is requested first (the in-order
/// vmcnt counter can then wait for it alone), and the rows are the one second-level load. The thread's
/// own row, its face, its gradient row's neighbour codes and (limited reconstructions) its own row's face
/// list are written without a branch, since a wait behind a divergent branch is a full one: a thread
/// without a row, face or gradient row reads entry 0 of its patch (a patch has a cell, a cell has faces)
/// and discards it. (gfx950, ROCm 7: the compiler folds the own and the ring row into one load of a
/// selected cell behind a wait for the id alone, and issues the codes before it; the dependent trips
/// before the first barrier are kernel arguments (two), record, id, rows -- profiles/r07/prologue_isa.md.)
/// The boundary look-ups of the neighbour codes (fz_gbf) stay lazy. The codes are loaded whether or not
/// the row's cell is owned: a ghost row holds four 0xFFFF codes (invariant of layout.cpp buildFused,
/// checked there), which decode to the -1s it takes.
template <bool MF, int LIM>
__device__ __forceinline__ void fz_load_first(const DevMesh& M, const SweepBuffers& B, const FzPatch& q, int t, FzPre& a)
{
	const bool own = t < q.nc, ring = !own && t < q.nl, grow = t < q.ng;
	int cr = 0;
	if(ring) cr = M.fz_ext[q.e0 + (t - q.nc)];
	const int co = q.c0 + (own ? t : 0);
	double uo[4];
	ld_state<MF>(B, co, uo);
	const double2 rco = M.rc[co];
	const int s = q.s0 + t;
	const bool face = s < q.s1;
	const int sc = face ? s : q.s0;
	const unsigned v = M.fz_slot_lr16[sc];    // R 0xFFFF: boundary face (bf from slot_LR)
	const double2 nn = M.slot_n[sc];
	const double len = M.slot_len[sc];
	const uint2 codes = q.gnbr[grow ? t : 0];
	int4 cs = make_int4(-1, -1, -1, -1);
	if(LIM) cs = M.cell_slots[co];
	a.cf = own ? co : cr;
	#pragma unroll
	for(int k = 0; k < 4; k++) a.ua[k] = uo[k];     // (a thread without a row stages nothing)
	a.rca = rco;
	if(ring) {
		ld_state<MF>(B, cr, a.ua);
		a.rca = M.rc[cr];
		if(LIM && grow && cr < M.nown) cs = M.cell_slots[cr];
	}
	a.lrl = make_int2(0, -1); a.nn = make_double2(0, 0); a.len = 0;
	if(face) {
		a.lrl = make_int2(static_cast<int>(v & 0xFFFFu), (v >> 16) == 0xFFFFu ? -2 : static_cast<int>(v >> 16));
		a.nn = nn; a.len = len;
	}
	a.nb4a = make_int4(-1, -1, -1, -1);
	if(grow) a.nb4a = fz_nbr_codes(codes, q.gbf);
	a.eps2a = 0.0;
	if(LIM) {   // the first row's face centres and eps^2, requested before the staging barrier
		// (owned gradient rows only: a ghost row's limiter values come with its gradient; the other
		// rows are left the patch's first cell's, which nothing reads)
		const bool og = grow && a.cf < M.nown;
		const int sl[4] = {cs.x, cs.y, cs.z, cs.w};
		#pragma unroll
		for(int k = 0; k < 4; k++) a.gpa[k] = sl[k] >= 0 ? M.slot_gr[sl[k] >> 1] : make_double2(0, 0);
		if(LIM == 2) a.eps2a = M.venk_eps2[og ? a.cf : 0];
	}
}

/// one patch (512 threads): phase 0 stages the primitive states and centres of the patch, ring-1 and
/// ring-2 cells in LDS; phase 1 computes the WLS gradients of the patch and ring-1 cells; phase 2 one
/// face per thread (reconstruction, flux, spectral radii); then the fluxes go through LDS and every
/// cell sums its faces in reference order. hookA runs at the start of phase 1, hookB after the face
/// work (points at which a caller may issue loads of later work).
template <int FLUX, int REC, bool DT, int VISC, int LIM, typename HA, typename HB>
__device__ __forceinline__ void fz_body(const DevMesh& M, const DevPhys& P, const SweepBuffers& B, double* fz,
                                        const FzPatch& q, const FzPre& a, HA&& hookA, HB&& hookB FZ_STAMPS_PARAM)
{
	const Gas& G = P.gas;
	const int t = static_cast<int>(threadIdx.x);
	const int s = q.s0 + t;
	constexpr int W = fz_w<VISC>();

	// phase 0: primitive states and centres of the staged cells
	if(t < q.nl) stage_row(G, &fz[t*W], a.ua, a.rca);
	for(int i = t + SLOTS_MAX; i < q.nl; i += SLOTS_MAX) {
		const int c = fz_cell(M, q, i);
		double b[4];
		ld_state<!DT>(B, c, b);
		stage_row(G, &fz[i*W], b, M.rc[c]);
	}
	FZ_STAMP(2);
	__syncthreads();
	FZ_STAMP(3);

	// phase 1: WLS gradients of the patch and ring-1 cells from the staged states
	// (k_prep_grad_wls arithmetic, neighbours in the same ascending reference face order)
	hookA();
	if(t < q.ng) fused_wls_row<LIM, W, !DT>(M, P, B, fz, &fz[t*W], a.cf, a.nb4a, LIM ? a.gpa : nullptr, a.eps2a);
	for(int i = t + SLOTS_MAX; i < q.ng; i += SLOTS_MAX) {
		const int c = fz_cell(M, q, i);
		fused_wls_row<LIM, W, !DT>(M, P, B, fz, &fz[i*W], c, c < M.nown ? fz_nbrs(q, i) : make_int4(-1, -1, -1, -1));
	}
	__syncthreads();
	FZ_STAMP(4);

	// phase 2: one face per thread (k_sweep arithmetic)
	double f[4] = {0, 0, 0, 0};
	double sri = 0, srj = 0;
	if(s < q.s1) {
		const int2 lrl = a.lrl;
		const double2 nn = a.nn;
		const double flen = a.len;
		const double n[2] = {nn.x, nn.y};
		const bool bnd = lrl.y < -1;
		int bf = 0, bcell = 0;          // boundary face: its index and cell from the global slot
		if(bnd) { const int2 g = M.slot_LR[s]; bf = g.y - M.ncell; bcell = g.x; }
		double ul[4], ur[4];
		const double* rowi = &fz[lrl.x*W];
		const double2 ri = *reinterpret_cast<const double2*>(rowi + 12);
		double ui[4], gi[8];
		ld4(rowi, 0, ui);
		ld8(rowi + 4, 0, gi);
		if(REC == SR_MUSCL) {
			if(!bnd) {
				const double* rowj = &fz[lrl.y*W];
				const double2 rj = *reinterpret_cast<const double2*>(rowj + 12);
				double uj[4], gj[8];
				ld4(rowj, 0, uj);
				ld8(rowj + 4, 0, gj);
				const double dx = rj.x-ri.x, dy = rj.y-ri.y;
				#pragma unroll
				for(int i = 0; i < 4; i++) {
					double dl = mul0(gi[i*2], dx); dl += gi[i*2+1]*dy;
					double dr = mul0(gj[i*2], dx); dr += gj[i*2+1]*dy;
					const double du = uj[i] - ui[i];
					const double dm = twice_minus(dl, du);
					const double dp = twice_minus(dr, du);
					ul[i] = muscl_left(ui[i], uj[i], dm, muscl_phi(dm, du));
					ur[i] = muscl_right(ui[i], uj[i], dp, muscl_phi(dp, du));
				}
				prim2cons(G, ul, ul);
				prim2cons(G, ur, ur);
			} else {
				// ghost of the cell value (k_prep_grad_wls / k_prep_bfaces arithmetic)
				const double4 gp = ghost_prim_of_cell<!DT>(M, P, B, bcell, bf);
				const double uj[4] = {gp.x, gp.y, gp.z, gp.w};
				const double2 rj = M.bf_rcbp[bf];
				const double dx = rj.x-ri.x, dy = rj.y-ri.y;
				#pragma unroll
				for(int i = 0; i < 4; i++) {
					double dl = mul0(gi[i*2], dx); dl += gi[i*2+1]*dy;
					const double du = uj[i] - ui[i];
					const double dm = twice_minus(dl, du);
					ul[i] = muscl_left(ui[i], uj[i], dm, muscl_phi(dm, du));
				}
				prim2cons(G, ul, ul);
				ghost_c(P, M.bf_bc[bf], ul, n, ur);
			}
		} else {  // unlimited linear
			const double2 gp = M.slot_gr[s];
			#pragma unroll
			for(int i = 0; i < 4; i++) {
				double v = ui[i];
				v += 1.0*gi[i*2]*(gp.x - ri.x);
				v += 1.0*gi[i*2+1]*(gp.y - ri.y);
				ul[i] = v;
			}
			prim2cons(G, ul, ul);
			if(!bnd) {
				const double* rowj = &fz[lrl.y*W];
				const double2 rj = *reinterpret_cast<const double2*>(rowj + 12);
				double uj[4], gj[8];
				ld4(rowj, 0, uj);
				ld8(rowj + 4, 0, gj);
				#pragma unroll
				for(int i = 0; i < 4; i++) {
					double v = uj[i];
					v += 1.0*gj[i*2]*(gp.x - rj.x);
					v += 1.0*gj[i*2+1]*(gp.y - rj.y);
					ur[i] = v;
				}
				prim2cons(G, ur, ur);
			} else {
				ghost_c(P, M.bf_bc[bf], ul, n, ur);
			}
		}
		inviscid_flux_len<FLUX>(G, ul, ur, n, flen, f);
		// Sutherland viscosities of the two face states: the time step's and the viscous flux's
		// (viscous_face_terms forms the same two values), formed once
		double mui = 0, muj = 0;
		if(VISC != SV_NONE) {
			mui = VISC == SV_CONST ? G.rReinf : sutherland(G, ul);
			muj = VISC == SV_CONST ? G.rReinf : sutherland(G, ur);
		}
		if(DT) {
			const double ci = sound_speed_cons(G, ul), cj = sound_speed_cons(G, ur);
			const double vni = div_rn(dot2(&ul[1],n), ul[0]);
			const double vnj = div_rn(dot2(&ur[1],n), ur[0]);
			sri = (fabs(vni)+ci)*flen;
			srj = (fabs(vnj)+cj)*flen;
			if(VISC != SV_NONE) {
				const double coi = visc_coef(G, ul[0]), coj = visc_coef(G, ur[0]);   // std::max(4/(3 rho), g/rho)
				// a ghost cell's spectral radius is never summed (and its area is not stored)
				const int2 g = M.slot_LR[s];
				if(g.x < M.nown) sri += div_rn(div_rcp(coi*mui, G.Pr, G.rPr) * flen*flen, M.area[g.x]);
				if(!bnd && g.y < M.nown) srj += div_rn(div_rcp(coj*muj, G.Pr, G.rPr) * flen*flen, M.area[g.y]);
			}
		}
		if(VISC != SV_NONE) {
			// modified-average viscous flux, k_sweep's arithmetic, from the staged primitive states,
			// gradients and centres; a boundary face takes its cell's ghost primitive state (B.ug of
			// the staged path) and the cell's own gradient. Register pressure: the face states enter
			// only through the averaged viscosity and velocity, formed first (the time step above has
			// used the face states too), and the fence makes the cell rows fresh LDS reads instead of
			// the reconstruction's copies kept live through the inviscid flux -- 4 waves per SIMD
			double muRe, va[2];
			viscous_face_terms_mu<VISC == SV_CONST>(G, ul, ur, mui, muj, muRe, va);
			double4 gpr = make_double4(0, 0, 0, 0);
			const double* rowj = nullptr;
			double2 rr;
			if(bnd) { gpr = ghost_prim_of_cell<!DT>(M, P, B, bcell, bf); rr = M.bf_rcbp[bf]; }
			else { rowj = &fz[lrl.y*W]; rr = *reinterpret_cast<const double2*>(rowj + 12); }
			const double4 vg = make_double4(ri.x, ri.y, rr.x, rr.y);    // the two centres
			double vf[4] = {0, 0, 0, 0};
			fz_viscous(G, rowi, rowj, gpr, vg, n, muRe, va, vf);
			#pragma unroll
			for(int k = 0; k < 4; k++) f[k] += vf[k]*flen;
		}
	}
	hookB();
	// the cell's face list (and area) are requested before the two barriers of the flux staging,
	// once the face work no longer holds registers
	const int c = q.c0 + t;
	uint2 cs = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
	double carea = 0.0;
	if(c < q.c1) { cs = M.fz_cslot16[c]; if(DT) carea = M.area[c]; }
	__syncthreads();   // all staged rows read: reuse LDS for the face fluxes
	double* sf = fz;
	double* ssr = fz + 4*SLOTS_MAX;
	if(s < q.s1) {
		sf[0*SLOTS_MAX + t] = f[0]; sf[1*SLOTS_MAX + t] = f[1];
		sf[2*SLOTS_MAX + t] = f[2]; sf[3*SLOTS_MAX + t] = f[3];
		if(DT) { ssr[t] = sri; ssr[SLOTS_MAX + t] = srj; }
	}
	__syncthreads();
	FZ_STAMP(5);

	if(c < q.c1) {
		double r[4];
		if(B.overwrite) { r[0] = r[1] = r[2] = r[3] = 0.0; }
		else ld4(B.r, c, r);
		double integ = 0.0;
		const unsigned e[4] = {cs.x & 0xFFFFu, cs.x >> 16, cs.y & 0xFFFFu, cs.y >> 16};
		#pragma unroll
		for(int k = 0; k < 4; k++) {
			if(e[k] == 0xFFFFu) break;
			const int ls = static_cast<int>(e[k] >> 1);     // patch-local slot
			if(e[k] & 1) {
				r[0] += sf[0*SLOTS_MAX + ls]; r[1] += sf[1*SLOTS_MAX + ls];
				r[2] += sf[2*SLOTS_MAX + ls]; r[3] += sf[3*SLOTS_MAX + ls];
				if(DT) integ += ssr[SLOTS_MAX + ls];
			} else {
				r[0] -= sf[0*SLOTS_MAX + ls]; r[1] -= sf[1*SLOTS_MAX + ls];
				r[2] -= sf[2*SLOTS_MAX + ls]; r[3] -= sf[3*SLOTS_MAX + ls];
				if(DT) integ += ssr[ls];
			}
		}
		if(!DT && B.mfx) {
			// y = mdt x + (-yg + res)/pert, k_mf_combine's arithmetic, with yg the sum just formed
			double x[4], rs[4];
			ld4(B.mfx, c, x);
			ld4(B.mfres, c, rs);
			const double d = B.mfmdt[c], pert = B.mfpm[1];
			#pragma unroll
			for(int i = 0; i < 4; i++) r[i] = d*x[i] + (-r[i] + rs[i])/pert;
		}
		st4(B.r, c, r);
		if(DT) B.dtm[c] = div_rn(carea, integ);
	}
	FZ_STAMP(6);
}

// waves per SIMD the fused instantiations are compiled for (VGPR budgets 96 / 128 / 168); the layout
// caps the staged rows to match (layout.cpp fusedRowCap: 5 blocks of 32 KB LDS per CU)
#ifndef FVHIP_FUSED_WAVES
#define FVHIP_FUSED_WAVES 5          // inviscid, unlimited: 90 VGPRs
#endif
#ifndef FVHIP_FUSED_WAVES_LIM
#define FVHIP_FUSED_WAVES_LIM 4      // Barth-Jespersen / Venkatakrishnan: 124-126 VGPRs
#endif
#ifndef FVHIP_FUSED_WAVES_VISC
#define FVHIP_FUSED_WAVES_VISC 4     // viscous: 110-122 VGPRs (fz_viscous streams the LDS rows; 144-156 before)
#endif

template <int FLUX, int REC, bool DT, int VISC, int LIM>
__global__ void __launch_bounds__(SLOTS_MAX, VISC != SV_NONE ? FVHIP_FUSED_WAVES_VISC : (LIM ? FVHIP_FUSED_WAVES_LIM : FVHIP_FUSED_WAVES)) k_residual_wls(const DevMesh M, const DevPhys P, const SweepBuffers B)
{
	extern __shared__ __attribute__((aligned(16))) double fz[];
#ifdef FVHIP_FZ_STAMPS
	FzStamps stamps;
	asm("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamps.w0) : "s"(blockIdx.y));
#endif
	FZ_STAMP_ENTRY();
	const int np = B.plist ? B.pcount : M.npatch;
	const int t = static_cast<int>(threadIdx.x);
	const int q = (np + 7) >> 3;
	const int pi = (blockIdx.x & 7) * q + (blockIdx.x >> 3);
	if(pi >= np) return;
	const FzPatch cur = fz_patch(M, B, pi);
	FZ_STAMP_AFTER(1, cur.s1, cur.nl, cur.ng, cur.c0);
	FzPre pre;
	fz_load_first<!DT, LIM>(M, B, cur, t, pre);
	fz_body<FLUX, REC, DT, VISC, LIM>(M, P, B, fz, cur, pre, []() {}, []() {} FZ_STAMPS_ARG);
#ifdef FVHIP_FZ_STAMPS
	if(t == 0 && B.stamps) {
		unsigned long long* o = B.stamps + 8*static_cast<size_t>(blockIdx.x);
		for(int k = 0; k < 7; k++) o[k] = stamps.t[k];
		o[7] = wall_clock64() - stamps.w0;
	}
#endif
}

// fused residual dispatch
typedef void (*FusedFn)(const DevMesh, const DevPhys, const SweepBuffers);
template <int FLUX, int VISC>
static FusedFn pickFused3(int rec, bool dt) {
	if(rec == SR_MUSCL) return dt ? k_residual_wls<FLUX,SR_MUSCL,true,VISC,0> : k_residual_wls<FLUX,SR_MUSCL,false,VISC,0>;
	return dt ? k_residual_wls<FLUX,SR_LINEAR,true,VISC,0> : k_residual_wls<FLUX,SR_LINEAR,false,VISC,0>;
}
/// lim: 0 none, 1 Barth-Jespersen, 2 Venkatakrishnan (inviscid; linear reconstruction of lim*g)
template <int FLUX>
static FusedFn pickFused(int rec, int visc, int lim, bool dt) {
	if(lim == 1) return dt ? k_residual_wls<FLUX,SR_LINEAR,true,SV_NONE,1> : k_residual_wls<FLUX,SR_LINEAR,false,SV_NONE,1>;
	if(lim == 2) return dt ? k_residual_wls<FLUX,SR_LINEAR,true,SV_NONE,2> : k_residual_wls<FLUX,SR_LINEAR,false,SV_NONE,2>;
	if(visc == SV_SUTHERLAND) return pickFused3<FLUX,SV_SUTHERLAND>(rec, dt);
	if(visc == SV_CONST) return pickFused3<FLUX,SV_CONST>(rec, dt);
	return pickFused3<FLUX,SV_NONE>(rec, dt);
}

static const char* kFusedNames[7] = FVHIP_FLUX_NAMES("k_residual_wls");

const char* launch_residual_wls(const DevMesh& M, const DevPhys& P, const SweepBuffers& B, int flux, int rec,
                                int visc, int lim, bool dt, hipStream_t s)
{
	const FusedFn fn = with_flux(flux, [&](auto F) { return pickFused<decltype(F)::value>(rec, visc, lim, dt); });
	const size_t W = visc != SV_NONE ? FZW_VISC : FZW;
	const size_t lds = std::max(static_cast<size_t>(M.fz_max_cells)*W, static_cast<size_t>(6*SLOTS_MAX))*sizeof(double);
	// raise the dynamic-LDS limit once per instantiation and device to the largest patch the layout
	// allows (hipFuncSetAttribute is a host-side runtime call: not on every launch)
	{
		static std::mutex mu;
		static std::set<std::pair<const void*, int>> configured;
		int dev = 0;
		if(hipGetDevice(&dev) != hipSuccess) throw std::runtime_error("k_residual_wls: hipGetDevice failed");
		std::lock_guard<std::mutex> lock(mu);
		if(configured.insert({reinterpret_cast<const void*>(fn), dev}).second) {
			const size_t maxlds = std::max(static_cast<size_t>(FUSED_LDS_CELLS)*W, static_cast<size_t>(6*SLOTS_MAX))*sizeof(double);
			const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
			                                         hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(maxlds));
			if(e != hipSuccess) {
				configured.erase({reinterpret_cast<const void*>(fn), dev});
				throw std::runtime_error(std::string("k_residual_wls: raising the dynamic LDS limit failed: ")
				                         + hipGetErrorString(e));
			}
		}
	}
	const int np = B.plist ? B.pcount : M.npatch;
	// (a mesh without owned cells has one patch without cells: nothing to sweep, and the kernel's idle
	// threads read entry 0 of their patch, which every patch of a mesh with cells has -- buildFused)
	if(np > 0 && M.nown > 0) hipLaunchKernelGGL(fn, dim3(8*((np + 7)/8)), dim3(SLOTS_MAX), lds, s, M, P, B);
	return kFusedNames[flux_index(flux)];
}

}
}
