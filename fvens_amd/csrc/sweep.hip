/** \file sweep.hip
 * \brief The staged face sweep of the MI355X residual (gfx950, wave64): k_sweep and its dispatch.
 *
 * Pipeline of one residual evaluation (FlowFV::compute_residual, flow_spatial.cpp:636-816); the per-cell
 * kernels are in gradients.hip, the one-launch form of the whole pipeline (k_residual_wls) in fused.hip:
 *   k_prep_cells   conserved -> primitive cell states                     (:697-699)
 *   k_prep_bfaces  boundary ghost state of the cell value, and its primitive (:679-695)
 *   k_grad_*       cell-centred primitive gradients (WLS / Green-Gauss)   (:704-708)
 *   k_limiter/k_weno  per-cell limiter values for limited reconstructions (:720-723)
 *   k_sweep        THE HOT KERNEL: per patch, every touching face is reconstructed, converted,
 *                  given its BC ghost if on the boundary, its inviscid (+viscous) flux and
 *                  spectral radii computed into LDS; then every cell of the patch sums its faces
 *                  from LDS in ascending reference face index and writes -r and the time step
 *                  (:731-812 incl. compute_fluxes :488-563 and compute_max_timestep :565-634).
 * No atomics: the per-cell sum order is the reference's single-thread order, so results are
 * deterministic and, with -ffp-contract=off, bitwise equal to it.
 */
#include "sweep_device.hpp"

namespace fvhip {
namespace FVHIP_NS {

/// Per-cell words (doubles) staged in LDS for a sweep variant, one 16-byte-aligned row per cell:
///   order 2: [up 4][reconstruction gradient 8][rc 2] (+[phi 4] if limiter); the viscous flux
///            takes its primitive states from up as well
///   order 1: [u 4] (+[rc 2] if viscous)
template <int REC, int VISC, bool PHI> struct Stage {
	static constexpr bool O2 = REC != SR_FIRST;
	static constexpr bool V = VISC != SV_NONE;
	static constexpr int UP = 0, RG = 4;
	static constexpr int RC = O2 ? 12 : 4;
	static constexpr int UC = 0;            // order 1 only
	static constexpr int PH = 14;
	static constexpr int W0 = O2 ? (14 + (PHI ? 4 : 0)) : (V ? 6 : 4);
	static constexpr int W = (W0 + 1) & ~1;
	static constexpr int BUF = (W > 6 ? W : 6) * SLOTS_MAX;   // flux staging reuses the buffer
};

template <int FLUX, int REC, int VISC, bool DT, bool PHI>
__global__ void __launch_bounds__(SLOTS_MAX) k_sweep(const DevMesh M, const DevPhys P, const SweepBuffers B)
{
	typedef Stage<REC, VISC, PHI> S;
	constexpr int W = S::W;
	__shared__ __attribute__((aligned(16))) double sbuf[S::BUF];

	// XCD-aware mapping: consecutive patches (which share halo cells) land on the same XCD
	const int np = B.plist ? B.pcount : M.npatch;
	const int q = (np + 7) >> 3;
	const int pi = (blockIdx.x & 7) * q + (blockIdx.x >> 3);
	if(pi >= np) return;
	const int p = B.plist ? B.plist[pi] : pi;
	const int s0 = M.patch_slot[p], s1 = M.patch_slot[p+1];
	const int c0 = M.patch_cell[p], c1 = M.patch_cell[p+1];
	const int nc = c1 - c0;
	const int N = M.ncell;
	const Gas& G = P.gas;
	const int t = static_cast<int>(threadIdx.x);

	// phase 0: stage the patch's own cells (contiguous range) with coalesced loads
	if(t < nc) {
		const int c = c0 + t;
		double* row = &sbuf[t*W];
		double a[8];
		if(S::O2) {
			ld4(B.up, c, a); st4(row + S::UP, 0, a);
			ld8(B.rgrad, c, a); st8(row + S::RG, 0, a);
			const double2 r = M.rc[c]; *reinterpret_cast<double2*>(row + S::RC) = r;
			if(PHI) { ld4(B.phi, c, a); st4(row + S::PH, 0, a); }
		} else {
			ld4(B.u, c, a); st4(row + S::UC, 0, a);
			if(S::V) { const double2 r = M.rc[c]; *reinterpret_cast<double2*>(row + S::RC) = r; }
		}
	}
	__syncthreads();

	// cell data from LDS when the cell is in this patch, else from global memory (halo). The LDS row
	// is read unconditionally (row 0 for a halo cell) and pinned in registers before the global
	// values may replace it, so the two never merge into one generic (flat) load
	auto inp = [&](int cell) { return static_cast<unsigned>(cell - c0) < static_cast<unsigned>(nc); };
	auto lrow = [&](int cell, int off) { return &sbuf[(inp(cell) ? cell - c0 : 0)*W + off]; };
	auto get4 = [&](int cell, int off, const double* g, double* o) {
		ld4(lrow(cell, off), 0, o);
		for(int k = 0; k < 4; k++) pin_regs(o[k]);
		if(!inp(cell)) ld4(g, cell, o);
	};
	auto get8 = [&](int cell, int off, const double* g, double* o) {
		ld8(lrow(cell, off), 0, o);
		for(int k = 0; k < 8; k++) pin_regs(o[k]);
		if(!inp(cell)) ld8(g, cell, o);
	};
	auto getrc = [&](int cell) -> double2 {
		double2 v = *reinterpret_cast<const double2*>(lrow(cell, S::RC));
		pin_regs(v.x); pin_regs(v.y);
		if(!inp(cell)) v = M.rc[cell];
		return v;
	};

	const int s = s0 + t;
	double f[4] = {0, 0, 0, 0};
	double sri = 0, srj = 0;
	if(s < s1) {
		const int2 lr = M.slot_LR[s];
		const double2 nn = M.slot_n[s];
		const double len = M.slot_len[s];
		const double n[2] = {nn.x, nn.y};
		const bool bnd = lr.y >= N;
		const int bf = lr.y - N;
		double ul[4], ur[4];

		if(REC == SR_FIRST) {
			get4(lr.x, S::UC, B.u, ul);
			if(bnd) ghost(P, M.bf_bc[bf], ul, n, ur);
			else    get4(lr.y, S::UC, B.u, ur);
		}
		else if(REC == SR_MUSCL) {
			const double2 ri = getrc(lr.x);
			double ui[4], gi[8];
			get4(lr.x, S::UP, B.up, ui);
			get8(lr.x, S::RG, B.rgrad, gi);
			if(!bnd) {
				const double2 rj = getrc(lr.y);
				double uj[4], gj[8];
				get4(lr.y, S::UP, B.up, uj);
				get8(lr.y, S::RG, B.rgrad, gj);
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
				const double2 rj = M.bf_rcbp[bf];
				double uj[4];
				ld4(B.ug, bf, uj);
				const double dx = rj.x-ri.x, dy = rj.y-ri.y;
				#pragma unroll
				for(int i = 0; i < 4; i++) {
					double dl = mul0(gi[i*2], dx); dl += gi[i*2+1]*dy;
					const double du = uj[i] - ui[i];
					const double dm = twice_minus(dl, du);
					ul[i] = muscl_left(ui[i], uj[i], dm, muscl_phi(dm, du));
				}
				prim2cons(G, ul, ul);
				ghost(P, M.bf_bc[bf], ul, n, ur);
			}
		}
		else {  // SR_LINEAR: unlimited, WENO-limited gradients or BJ/Venkatakrishnan limiter values
			const double2 gp = M.slot_gr[s];
			{
				const double2 ri = getrc(lr.x);
				double ui[4], gi[8], ph[4] = {1.0, 1.0, 1.0, 1.0};
				get4(lr.x, S::UP, B.up, ui);
				get8(lr.x, S::RG, B.rgrad, gi);
				if(PHI) get4(lr.x, S::PH, B.phi, ph);
				#pragma unroll
				for(int i = 0; i < 4; i++) {
					double v = ui[i];
					v += ph[i]*gi[i*2]*(gp.x - ri.x);
					v += ph[i]*gi[i*2+1]*(gp.y - ri.y);
					ul[i] = v;
				}
				prim2cons(G, ul, ul);
			}
			if(!bnd) {
				const double2 rj = getrc(lr.y);
				double uj[4], gj[8], ph[4] = {1.0, 1.0, 1.0, 1.0};
				get4(lr.y, S::UP, B.up, uj);
				get8(lr.y, S::RG, B.rgrad, gj);
				if(PHI) get4(lr.y, S::PH, B.phi, ph);
				#pragma unroll
				for(int i = 0; i < 4; i++) {
					double v = uj[i];
					v += ph[i]*gj[i*2]*(gp.x - rj.x);
					v += ph[i]*gj[i*2+1]*(gp.y - rj.y);
					ur[i] = v;
				}
				prim2cons(G, ur, ur);
			} else {
				ghost(P, M.bf_bc[bf], ul, n, ur);
			}
		}

		inviscid_flux_len<FLUX>(G, ul, ur, n, len, f);

		if(VISC != SV_NONE) {
			// order 2: primitive states (up / ghost ug); order 1: conserved states
			double ucl[4], ucr[4], gl[8], gr[8];
			const double2 rl = getrc(lr.x);
			double2 rr;
			if(REC == SR_FIRST) get4(lr.x, S::UC, B.u, ucl);
			else get4(lr.x, S::UP, B.up, ucl);
			if(bnd) {
				rr = M.bf_rcbp[bf];
				if(REC == SR_FIRST) { for(int k = 0; k < 4; k++) ucr[k] = ur[k]; }
				else ld4(B.ug, bf, ucr);
			} else {
				rr = getrc(lr.y);
				if(REC == SR_FIRST) get4(lr.y, S::UC, B.u, ucr);
				else get4(lr.y, S::UP, B.up, ucr);
			}
			if(REC != SR_FIRST) {
				const int cr = bnd ? lr.x : lr.y;
				if(B.grad == B.rgrad) { get8(lr.x, S::RG, B.grad, gl); get8(cr, S::RG, B.grad, gr); }
				else { ld8(B.grad, lr.x, gl); ld8(B.grad, cr, gr); }
			}
			const double rcl[2] = {rl.x, rl.y}, rcr[2] = {rr.x, rr.y};
			double vf[4];
			viscous_flux<REC != SR_FIRST, VISC == SV_CONST>(G, n, rcl, rcr, ucl, ucr, gl, gr, ul, ur, vf);
			#pragma unroll
			for(int k = 0; k < 4; k++) f[k] += vf[k]*len;
		}

		if(DT) {
			const double ci = sound_speed_cons(G, ul), cj = sound_speed_cons(G, ur);
			const double vni = div_rn(dot2(&ul[1],n), ul[0]);
			const double vnj = div_rn(dot2(&ur[1],n), ur[0]);
			sri = (fabs(vni)+ci)*len;
			srj = (fabs(vnj)+cj)*len;
			if(VISC != SV_NONE) {
				const double mui = VISC == SV_CONST ? G.rReinf : sutherland(G, ul);
				const double muj = VISC == SV_CONST ? G.rReinf : sutherland(G, ur);
				const double coi = visc_coef(G, ul[0]), coj = visc_coef(G, ur[0]);   // std::max(4/(3 rho), g/rho)
				// a ghost cell's spectral radius is never summed (and its area is not stored)
				if(lr.x < M.nown) sri += div_rn(div_rcp(coi*mui, G.Pr, G.rPr) * len*len, M.area[lr.x]);
				if(!bnd && lr.y < M.nown) srj += div_rn(div_rcp(coj*muj, G.Pr, G.rPr) * len*len, M.area[lr.y]);
			}
		}
	}
	// the cell's face list (and area) are requested before the two barriers of the flux staging,
	// once the face work no longer holds registers
	const int c = c0 + t;
	int4 cs = make_int4(-1, -1, -1, -1);
	double carea = 0.0;
	if(c < c1) { cs = M.cell_slots[c]; if(DT) carea = M.area[c]; }
	__syncthreads();   // every slot has read the staged cells: reuse the buffer for the fluxes
	double* sf = sbuf;                  // [4][SLOTS_MAX]
	double* ssr = sbuf + 4*SLOTS_MAX;   // [2][SLOTS_MAX]
	if(s < s1) {
		sf[0*SLOTS_MAX + t] = f[0]; sf[1*SLOTS_MAX + t] = f[1];
		sf[2*SLOTS_MAX + t] = f[2]; sf[3*SLOTS_MAX + t] = f[3];
		if(DT) { ssr[t] = sri; ssr[SLOTS_MAX + t] = srj; }
	}
	__syncthreads();

	if(c < c1) {
		double r[4];
		if(B.overwrite) { r[0] = r[1] = r[2] = r[3] = 0.0; }
		else ld4(B.r, c, r);
		double integ = 0.0;
		const int e[4] = {cs.x, cs.y, cs.z, cs.w};
		#pragma unroll
		for(int k = 0; k < 4; k++) {
			if(e[k] < 0) break;
			const int ls = (e[k] >> 1) - s0;
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
		st4(B.r, c, r);
		if(DT) B.dtm[c] = div_rn(carea, integ);
	}
}

// sweep dispatch over (flux, reconstruction, viscous, dt, phi)
typedef void (*SweepFn)(const DevMesh, const DevPhys, const SweepBuffers);

template <int FLUX, int REC, int VISC>
static SweepFn pick4(bool dt, bool phi) {
	if(REC == SR_LINEAR) {
		if(dt) return phi ? k_sweep<FLUX,REC,VISC,true,true> : k_sweep<FLUX,REC,VISC,true,false>;
		return phi ? k_sweep<FLUX,REC,VISC,false,true> : k_sweep<FLUX,REC,VISC,false,false>;
	}
	return dt ? k_sweep<FLUX,REC,VISC,true,false> : k_sweep<FLUX,REC,VISC,false,false>;
}
template <int FLUX, int REC>
static SweepFn pick3(int visc, bool dt, bool phi) {
	switch(visc) {
		case SV_NONE: return pick4<FLUX,REC,SV_NONE>(dt, phi);
		case SV_SUTHERLAND: return pick4<FLUX,REC,SV_SUTHERLAND>(dt, phi);
		default: return pick4<FLUX,REC,SV_CONST>(dt, phi);
	}
}
template <int FLUX>
static SweepFn pick2(int rec, int visc, bool dt, bool phi) {
	switch(rec) {
		case SR_FIRST: return pick3<FLUX,SR_FIRST>(visc, dt, phi);
		case SR_MUSCL: return pick3<FLUX,SR_MUSCL>(visc, dt, phi);
		default: return pick3<FLUX,SR_LINEAR>(visc, dt, phi);
	}
}

static const char* kSweepNames[7] = FVHIP_FLUX_NAMES("k_sweep");

const char* launch_sweep(const DevMesh& M, const DevPhys& P, const SweepBuffers& B, int flux, int rec,
                         int visc, bool dt, hipStream_t s)
{
	const bool phi = B.phi != nullptr;
	const SweepFn fn = with_flux(flux, [&](auto F) { return pick2<decltype(F)::value>(rec, visc, dt, phi); });
	const int np = B.plist ? B.pcount : M.npatch;
	if(np > 0) hipLaunchKernelGGL(fn, dim3(8*((np + 7)/8)), dim3(SLOTS_MAX), 0, s, M, P, B);
	return kSweepNames[flux_index(flux)];
}

}
}
