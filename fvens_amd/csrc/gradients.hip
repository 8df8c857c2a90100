/** \file gradients.hip
 * \brief The per-cell HIP kernels of the face sweep (gfx950, wave64) and their launchers: preparation,
 *   WLS and Green-Gauss gradients, limiters, WENO, fill, gather / scatter and the probes. Where they
 *   stand in a residual evaluation: the pipeline in sweep.hip.
 */
#include "sweep_device.hpp"
#include <stdexcept>

namespace fvhip {
namespace FVHIP_NS {

// ------------------------------------------------------------------------------------------------
// preparation
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_prep_cells(int N, Gas G, const double* __restrict__ u, double* __restrict__ up)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= N) return;
	double a[4], b[4];
	ld4(u, c, a);
	cons2prim(G, a, b);
	st4(up, c, b);
}

__global__ void __launch_bounds__(256) k_prep_bfaces(DevMesh M, DevPhys P, const double* __restrict__ u,
                                                     double* __restrict__ ubc, double* __restrict__ ug)
{
	const int f = blockIdx.x*blockDim.x + threadIdx.x;
	if(f >= M.nbface) return;
	double a[4], g[4], p[4];
	ld4(u, M.bf_L[f], a);
	const double2 nn = M.bf_n[f];
	const double n[2] = {nn.x, nn.y};
	ghost_state(P.gas, P.bc[M.bf_bc[f]], P.uinf, a, n, g);
	st4(ubc, f, g);
	cons2prim(P.gas, g, p);
	st4(ug, f, p);
}

// ------------------------------------------------------------------------------------------------
// gradients (agradientschemes.cpp). One thread per cell; the cell's faces are visited in ascending
// reference face index, which is the reference's single-thread accumulation order.
// ------------------------------------------------------------------------------------------------
// WLS (agradientschemes.cpp:322-440). Each face contributes w2*dr*du with dr = rc(L)-rc(R),
// du = u(L)-u(R); computing both differences from this cell's side negates both factors exactly,
// so the product is bitwise the same and no face orientation is needed.
// (The accumulation is spelt out in each of the four WLS kernels here and in fused.hip's boundary branch:
// moved into a shared helper, by value or by reference, it changed the machine code of all of them.)
__global__ void __launch_bounds__(256) k_grad_wls(DevMesh M, const double* __restrict__ up,
                                                  const double* __restrict__ ug, double* __restrict__ grad)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= M.nown) return;
	const int N = M.ncell;     // cells incl. ghosts: codes >= N are boundary faces
	const int4 nb4 = M.cell_nbr_fo[c];
	const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
	const double2 rcc = M.rc[c];
	double uc[4];
	ld4(up, c, uc);
	// issue all neighbour loads before the arithmetic
	double un[4][4];
	double2 rn[4];
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(nb[k] < 0) continue;
		if(nb[k] >= N) { rn[k] = M.bf_rcbp[nb[k] - N]; ld4(ug, nb[k] - N, un[k]); }
		else           { rn[k] = M.rc[nb[k]];           ld4(up, nb[k], un[k]); }
	}
	const double4 V = M.wls_V[c];
	double f[8] = {0,0,0,0,0,0,0,0};
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(nb[k] < 0) break;
		double w2 = 0;
		w2 += (rcc.x-rn[k].x)*(rcc.x-rn[k].x);
		w2 += (rcc.y-rn[k].y)*(rcc.y-rn[k].y);
		const double dr0 = rcc.x-rn[k].x, dr1 = rcc.y-rn[k].y;
		w2 = div_rn(1.0, w2);
		#pragma unroll
		for(int iv = 0; iv < 4; iv++) {
			const double du = uc[iv] - un[k][iv];
			f[iv*2+0] += w2*dr0*du;
			f[iv*2+1] += w2*dr1*du;
		}
	}
	double g[8];
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) {
		g[iv*2+0] = V.x*f[iv*2+0] + V.y*f[iv*2+1];
		g[iv*2+1] = V.z*f[iv*2+0] + V.w*f[iv*2+1];
	}
	st8(grad, c, g);
}

/// Fused preparation + WLS gradient for the residual path: converts this cell's conserved state
/// (written as up[c]) and its neighbours' (k_prep_cells' cons2prim, bit for bit), builds the ghost
/// states of this cell's boundary faces (k_prep_bfaces; each boundary face has exactly one cell),
/// then the same WLS arithmetic as k_grad_wls. A block owns 256 consecutive (Hilbert-ordered)
/// cells; their primitive states and centres are staged in LDS, so only neighbours outside the
/// block are gathered from global memory.
/// LIM (1 Barth-Jespersen, 2 Venkatakrishnan): the cell's limiter values follow from the same
/// neighbour states with k_limiter's arithmetic (face centres in reference face order from
/// cell_slots), so the separate limiter pass and its re-reads disappear
template <int LIM>
__global__ void __launch_bounds__(256) k_prep_grad_wls(DevMesh M, DevPhys P, const double* __restrict__ u,
                                                       double* __restrict__ up, double* __restrict__ ubc,
                                                       double* __restrict__ ug, double* __restrict__ grad,
                                                       int c_begin, int c_end, double* __restrict__ phi)
{
	__shared__ __attribute__((aligned(16))) double s_up[256][4];
	__shared__ __attribute__((aligned(16))) double2 s_rc[256];
	const int N = M.ncell;        // owned + ghost: neighbour codes >= N are boundary faces
	const int NO = c_end;         // this launch's cells: [c_begin, c_end) of the owned cells
	const int cb = c_begin + xcd_chunk(static_cast<int>((c_end - c_begin + 255) >> 8))*256;
	if(cb >= NO) return;
	const int t = static_cast<int>(threadIdx.x);
	const int c = cb + t;
	const int ncb = (NO - cb) < 256 ? (NO - cb) : 256;
	const Gas& G = P.gas;
	double ucons[4], uc[4];
	double2 rcc = make_double2(0, 0);
	if(c < NO) {
		ld4(u, c, ucons);
		cons2prim(G, ucons, uc);
		st4(up, c, uc);
		rcc = M.rc[c];
		st4(&s_up[t][0], 0, uc);
		s_rc[t] = rcc;
	}
	__syncthreads();
	if(c >= NO) return;
	const int4 nb4 = M.cell_nbr_fo[c];
	const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
	double un[4][4];
	double2 rn[4];
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(nb[k] < 0) continue;
		const int j = nb[k] - cb;
		if(static_cast<unsigned>(j) < static_cast<unsigned>(ncb)) {
			ld4(&s_up[j][0], 0, un[k]);
			rn[k] = s_rc[j];
		} else if(nb[k] >= N) {
			const int bf = nb[k] - N;
			const double2 nn = M.bf_n[bf];
			const double n[2] = {nn.x, nn.y};
			double gs[4];
			ghost(P, M.bf_bc[bf], ucons, n, gs);
			st4(ubc, bf, gs);
			cons2prim(G, gs, un[k]);
			st4(ug, bf, un[k]);
			rn[k] = M.bf_rcbp[bf];
		} else {
			double t4[4];
			ld4(u, nb[k], t4);
			rn[k] = M.rc[nb[k]];
			cons2prim(G, t4, un[k]);
		}
	}
	const double4 V = M.wls_V[c];
	double f[8] = {0,0,0,0,0,0,0,0};
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(nb[k] < 0) break;
		double w2 = 0;
		w2 += (rcc.x-rn[k].x)*(rcc.x-rn[k].x);
		w2 += (rcc.y-rn[k].y)*(rcc.y-rn[k].y);
		const double dr0 = rcc.x-rn[k].x, dr1 = rcc.y-rn[k].y;
		w2 = div_rn(1.0, w2);
		#pragma unroll
		for(int iv = 0; iv < 4; iv++) {
			const double du = uc[iv] - un[k][iv];
			f[iv*2+0] += w2*dr0*du;
			f[iv*2+1] += w2*dr1*du;
		}
	}
	double g[8];
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) {
		g[iv*2+0] = V.x*f[iv*2+0] + V.y*f[iv*2+1];
		g[iv*2+1] = V.z*f[iv*2+0] + V.w*f[iv*2+1];
	}
	st8(grad, c, g);
	if(LIM) {
		const int4 cs = M.cell_slots[c];
		const int sl[4] = {cs.x, cs.y, cs.z, cs.w};
		double2 gp[4];
		bool has[4];
		#pragma unroll
		for(int k = 0; k < 4; k++) {
			has[k] = nb[k] >= 0;
			if(has[k]) gp[k] = M.slot_gr[sl[k] >> 1];
		}
		double out[4];
		cell_limiter<LIM == 2>(uc, g, un, gp, has, rcc, LIM == 2 ? M.venk_eps2[c] : 0.0, out);
		st4(phi, c, out);
	}
}

/// WLS gradients of a list of owned cells (the cells other ranks hold as ghosts), all inputs from
/// global memory: same arithmetic as k_prep_grad_wls, written to grad for the halo exchange
__global__ void __launch_bounds__(256) k_grad_wls_list(DevMesh M, DevPhys P, const double* __restrict__ u,
                                                       const int* __restrict__ list, int n, double* __restrict__ grad)
{
	const int i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n) return;
	const int c = list[i];
	const int N = M.ncell;
	const Gas& G = P.gas;
	const int4 nb4 = M.cell_nbr_fo[c];
	const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
	double ucons[4], uc[4];
	ld4(u, c, ucons);
	cons2prim(G, ucons, uc);
	const double2 rcc = M.rc[c];
	double f[8] = {0,0,0,0,0,0,0,0};
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(nb[k] < 0) break;
		double un[4];
		double2 rn;
		if(nb[k] >= N) {
			const int bf = nb[k] - N;
			const double2 nn = M.bf_n[bf];
			const double n[2] = {nn.x, nn.y};
			double gs[4];
			ghost(P, M.bf_bc[bf], ucons, n, gs);
			cons2prim(G, gs, un);
			rn = M.bf_rcbp[bf];
		} else {
			double t4[4];
			ld4(u, nb[k], t4);
			cons2prim(G, t4, un);
			rn = M.rc[nb[k]];
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
	}
	const double4 V = M.wls_V[c];
	double g[8];
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) {
		g[iv*2+0] = V.x*f[iv*2+0] + V.y*f[iv*2+1];
		g[iv*2+1] = V.z*f[iv*2+0] + V.w*f[iv*2+1];
	}
	st8(grad, c, g);
}

/// WLS gradients of the layer-1 ghosts of a two-layer halo, from the received layer-1 and layer-2
/// states: the arithmetic of k_grad_wls_list on the ghost's own neighbour list (ascending global face
/// order; extra boundary faces for the physical faces no owned cell touches), so each value is the
/// owner's bit for bit and needs no exchange. LIM (1 Barth-Jespersen, 2 Venkatakrishnan): the ghost's
/// limiter values too, k_prep_grad_wls<LIM>'s cell_limiter on the same neighbour states (boundary:
/// the ghost primitive state) and the ghost's face centres -- the owner's values, since min / max over
/// the faces do not depend on their order (limitedlinearreconstruction.cpp:107-268)
template <int LIM>
__global__ void __launch_bounds__(256) k_grad_ghost(DevMesh M, DevPhys P, const double* __restrict__ u,
                                                    double* __restrict__ grad, double* __restrict__ phi)
{
	const int i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= M.gg_n) return;
	const int c = M.gg_cells[i];
	const Gas& G = P.gas;
	const int4 nb4 = M.gg_nbr[i];
	const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
	// every row this ghost reads is requested at once (a second dependent round trip after the cell
	// and neighbour ids), not one neighbour after another: the kernel is latency-bound (a few
	// thousand ghosts per rank) and sits on the halo's critical path
	double ucons[4], uc[4];
	ld4(u, c, ucons);
	const double2 rcc = M.rc[c];
	double t4[4][4];
	double2 rn4[4];
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		const int j = nb[k] >= 0 ? nb[k] : c;
		ld4(u, j, t4[k]);
		rn4[k] = M.rc[j];
	}
	cons2prim(G, ucons, uc);
	double f[8] = {0,0,0,0,0,0,0,0};
	double un[4][4];
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(nb[k] == -1) break;
		double2 rn;
		if(nb[k] < 0) {
			const int x = -2 - nb[k];
			const double2 nn = M.xb_n[x];
			const double n[2] = {nn.x, nn.y};
			double gs[4];
			ghost(P, M.xb_bc[x], ucons, n, gs);
			cons2prim(G, gs, un[k]);
			rn = M.xb_rcbp[x];
		} else {
			cons2prim(G, t4[k], un[k]);
			rn = rn4[k];
		}
		double w2 = 0;
		w2 += (rcc.x-rn.x)*(rcc.x-rn.x);
		w2 += (rcc.y-rn.y)*(rcc.y-rn.y);
		const double dr0 = rcc.x-rn.x, dr1 = rcc.y-rn.y;
		w2 = div_rn(1.0, w2);
		#pragma unroll
		for(int iv = 0; iv < 4; iv++) {
			const double du = uc[iv] - un[k][iv];
			f[iv*2+0] += w2*dr0*du;
			f[iv*2+1] += w2*dr1*du;
		}
	}
	const double4 V = M.gg_V[i];
	double g[8];
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) {
		g[iv*2+0] = V.x*f[iv*2+0] + V.y*f[iv*2+1];
		g[iv*2+1] = V.z*f[iv*2+0] + V.w*f[iv*2+1];
	}
	st8(grad, c, g);
	if(LIM) {
		double2 gp[4];
		bool has[4];
		#pragma unroll
		for(int k = 0; k < 4; k++) {
			has[k] = nb[k] != -1;
			gp[k] = M.gg_gp[4*i + k];
		}
		double out[4];
		cell_limiter<LIM == 2>(uc, g, un, gp, has, rcc, LIM == 2 ? M.gg_eps2[i] : 0.0, out);
		st4(phi, c, out);
	}
}

__global__ void __launch_bounds__(256) k_grad_gg(DevMesh M, const double* __restrict__ up,
                                                 const double* __restrict__ ug, double* __restrict__ grad)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= M.nown) return;
	const int N = M.ncell;     // cells incl. ghosts: codes >= N are boundary faces
	const int4 cs = M.cell_slots[c];
	const int e[4] = {cs.x, cs.y, cs.z, cs.w};
	double g[8] = {0,0,0,0,0,0,0,0};
	const double ainv = div_rn(1.0, M.area[c]);
	#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(e[k] < 0) break;
		const int s = e[k] >> 1;
		const int2 lr = M.slot_LR[s];
		const double2 mid = M.slot_gr[s];
		const double2 nn = M.slot_n[s];
		const double len = M.slot_len[s];
		double uL[4], uR[4];
		const double2 rl = M.rc[lr.x];
		double2 rr;
		ld4(up, lr.x, uL);
		if(lr.y >= N) { rr = M.bf_rcbp[lr.y - N]; ld4(ug, lr.y - N, uR); }
		else          { rr = M.rc[lr.y];           ld4(up, lr.y, uR); }
		double dL = 0, dR = 0;
		dL += (mid.x-rl.x)*(mid.x-rl.x); dR += (mid.x-rr.x)*(mid.x-rr.x);
		dL += (mid.y-rl.y)*(mid.y-rl.y); dR += (mid.y-rr.y)*(mid.y-rr.y);
		dL = div_rn(1.0, sqrt_rn(dL));
		dR = div_rn(1.0, sqrt_rn(dR));
		const bool right = e[k] & 1;
		#pragma unroll
		for(int iv = 0; iv < 4; iv++) {
			const double ut = div_rn(uL[iv]*dL + uR[iv]*dR, dL+dR) * len;
			if(!right) { g[iv*2+0] += (ut*nn.x)*ainv; g[iv*2+1] += (ut*nn.y)*ainv; }
			else       { g[iv*2+0] -= (ut*nn.x)*ainv; g[iv*2+1] -= (ut*nn.y)*ainv; }
		}
	}
	st8(grad, c, g);
}

// ------------------------------------------------------------------------------------------------
// limiters (limitedlinearreconstruction.cpp:107-268). Physical-boundary neighbours use the ghost
// primitive state (documented deviation: the reference reads past the end of its array there).
// ------------------------------------------------------------------------------------------------
template <bool VENK>
__global__ void __launch_bounds__(256) k_limiter(DevMesh M, const double* __restrict__ up, const double* __restrict__ ug,
                                                 const double* __restrict__ grad, double* __restrict__ phi)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= M.nown) return;
	const int N = M.ncell;     // cells incl. ghosts: codes >= N are boundary faces
	double uc[4], g[8];
	ld4(up, c, uc);
	ld8(grad, c, g);
	const int4 nb4 = M.cell_nbr[c], fs4 = M.cell_face[c];
	const int nbr[4] = {nb4.x, nb4.y, nb4.z, nb4.w}, fcs[4] = {fs4.x, fs4.y, fs4.z, fs4.w};
	const double2 r = M.rc[c];
	const double eps2 = VENK ? M.venk_eps2[c] : 0.0;
	double un[4][4];
	double2 gp[4];
	#pragma unroll
	for(int j = 0; j < 4; j++) {
		if(nbr[j] < 0) continue;
		if(nbr[j] >= N) ld4(ug, nbr[j]-N, un[j]); else ld4(up, nbr[j], un[j]);
		gp[j] = M.slot_gr[fcs[j]];
	}
	const bool has[4] = {nbr[0] >= 0, nbr[1] >= 0, nbr[2] >= 0, nbr[3] >= 0};
	double out[4];
	cell_limiter<VENK>(uc, g, un, gp, has, r, eps2, out);
	st4(phi, c, out);
}

// WENO-limited gradients (limitedlinearreconstruction.cpp:27-105)
__global__ void __launch_bounds__(256) k_weno(DevMesh M, double lambda, const double* __restrict__ grad,
                                              double* __restrict__ lgrad)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= M.nown) return;
	const int N = M.ncell;     // cells incl. ghosts: codes >= N are boundary faces
	const double gamma = 4.0, epsilon = 1.0e-5;
	double g0[8];
	ld8(grad, c, g0);
	const int4 nb4 = M.cell_nbr[c];
	const int nbr[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
	double gn[4][8];
	#pragma unroll
	for(int j = 0; j < 4; j++) if(nbr[j] >= 0 && nbr[j] < N) ld8(grad, nbr[j], gn[j]);
	double out[8];
	#pragma unroll
	for(int iv = 0; iv < 4; iv++) {
		double wsum = 0, l0 = 0, l1 = 0;
		{
			double m2 = 0; m2 += g0[iv*2]*g0[iv*2]; m2 += g0[iv*2+1]*g0[iv*2+1];
			const double w = lambda / pow(m2 + epsilon, gamma);
			wsum += w; l0 += w*g0[iv*2]; l1 += w*g0[iv*2+1];
		}
		#pragma unroll
		for(int j = 0; j < 4; j++) {
			if(nbr[j] < 0 || nbr[j] >= N) continue;
			double m2 = 0; m2 += gn[j][iv*2]*gn[j][iv*2]; m2 += gn[j][iv*2+1]*gn[j][iv*2+1];
			const double w = 1.0 / pow(m2 + epsilon, gamma);
			wsum += w; l0 += w*gn[j][iv*2]; l1 += w*gn[j][iv*2+1];
		}
		out[iv*2] = l0/wsum; out[iv*2+1] = l1/wsum;
	}
	st8(lgrad, c, out);
}

// ------------------------------------------------------------------------------------------------
// misc
// ------------------------------------------------------------------------------------------------
__global__ void k_fill(double* p, double v, long long n)
{
	const long long i = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	if(i < n) p[i] = v;
}

__global__ void k_local_flux(int type, Gas G, int nf, const double* ul, const double* ur, const double* n, double* f)
{
	const int i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= nf) return;
	double a[4], b[4], o[4];
	ld4(ul, i, a); ld4(ur, i, b);
	const double nn[2] = {n[2*i], n[2*i+1]};
	inviscid_flux_rt(type, G, a, b, nn, o);
	st4(f, i, o);
}

__global__ void k_gather(const int* perm, const double* src, double* dst, int n, int width)
{
	const long long i = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	if(i >= static_cast<long long>(n)*width) return;
	const int c = static_cast<int>(i / width), w = static_cast<int>(i % width);
	dst[i] = src[static_cast<size_t>(perm[c])*width + w];
}

/// dst row perm[c] = src row c (internal -> reference order, the inverse of k_gather)
__global__ void k_scatter(const int* perm, const double* src, double* dst, int n, int width)
{
	const long long i = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	if(i >= static_cast<long long>(n)*width) return;
	const int c = static_cast<int>(i / width), w = static_cast<int>(i % width);
	dst[static_cast<size_t>(perm[c])*width + w] = src[i];
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
void launch_prep(const DevMesh& M, const DevPhys& P, const double* u, double* up, double* ubc, double* ug,
                 bool cells, hipStream_t s)
{
	if(cells && M.nown > 0) k_prep_cells<<<nblk(M.nown,256), 256, 0, s>>>(M.nown, P.gas, u, up);
	if(M.nbface > 0) k_prep_bfaces<<<nblk(M.nbface,256), 256, 0, s>>>(M, P, u, ubc, ug);
}
void launch_grad_wls(const DevMesh& M, const double* up, const double* ug, double* grad, hipStream_t s)
{ if(M.nown > 0) k_grad_wls<<<nblk(M.nown,256), 256, 0, s>>>(M, up, ug, grad); }
void launch_prep_grad_wls(const DevMesh& M, const DevPhys& P, const double* u, double* up, double* ubc,
                          double* ug, double* grad, hipStream_t s, int c_begin, int c_end, int lim, double* phi)
{
	if(c_end < 0) c_end = M.nown;
	if(c_end <= c_begin) return;
	const dim3 g(xcd_blocks((c_end - c_begin + 255)/256)), b(256);
	if(lim == 1) k_prep_grad_wls<1><<<g, b, 0, s>>>(M, P, u, up, ubc, ug, grad, c_begin, c_end, phi);
	else if(lim == 2) k_prep_grad_wls<2><<<g, b, 0, s>>>(M, P, u, up, ubc, ug, grad, c_begin, c_end, phi);
	else k_prep_grad_wls<0><<<g, b, 0, s>>>(M, P, u, up, ubc, ug, grad, c_begin, c_end, phi);
}
void launch_grad_wls_list(const DevMesh& M, const DevPhys& P, const double* u, const int* list, int n,
                          double* grad, hipStream_t s)
{ if(n > 0) k_grad_wls_list<<<nblk(n,256), 256, 0, s>>>(M, P, u, list, n, grad); }
void launch_grad_gg(const DevMesh& M, const double* up, const double* ug, double* grad, hipStream_t s)
{ if(M.nown > 0) k_grad_gg<<<nblk(M.nown,256), 256, 0, s>>>(M, up, ug, grad); }
void launch_limiter(const DevMesh& M, const DevPhys& P, int venk, const double* up, const double* ug,
                    const double* grad, double* phi, hipStream_t s)
{
	if(M.nown <= 0) return;
	if(venk) k_limiter<true><<<nblk(M.nown,256), 256, 0, s>>>(M, up, ug, grad, phi);
	else     k_limiter<false><<<nblk(M.nown,256), 256, 0, s>>>(M, up, ug, grad, phi);
}

void launch_grad_ghost(const DevMesh& M, const DevPhys& P, const double* u, double* grad, hipStream_t s, int lim, double* phi)
{
	if(M.gg_n <= 0) return;
	if(lim && !phi) throw std::invalid_argument("launch_grad_ghost: limiter values need a phi buffer");
	if(lim == 2 && !M.gg_eps2) throw std::invalid_argument("launch_grad_ghost: Venkatakrishnan eps^2 of the ghosts missing");
	if(lim && !M.gg_gp) throw std::invalid_argument("launch_grad_ghost: ghost face centres missing");
	const int nb = (M.gg_n + 255)/256;
	if(lim == 2) k_grad_ghost<2><<<nb, 256, 0, s>>>(M, P, u, grad, phi);
	else if(lim == 1) k_grad_ghost<1><<<nb, 256, 0, s>>>(M, P, u, grad, phi);
	else k_grad_ghost<0><<<nb, 256, 0, s>>>(M, P, u, grad, phi);
}
void launch_weno(const DevMesh& M, const DevPhys& P, const double* grad, double* lgrad, hipStream_t s)
{ if(M.nown > 0) k_weno<<<nblk(M.nown,256), 256, 0, s>>>(M, P.limiter_param, grad, lgrad); }
void launch_fill(double* p, double v, long long n, hipStream_t s)
{ if(n > 0) k_fill<<<nblk(n,256), 256, 0, s>>>(p, v, n); }
void launch_local_flux(int flux, const Gas& G, int nf, const double* ul, const double* ur,
                       const double* n, double* f, hipStream_t s)
{ if(nf > 0) k_local_flux<<<nblk(nf,256), 256, 0, s>>>(flux, G, nf, ul, ur, n, f); }
/// parity-mode division and square root against the device's IEEE a/b and sqrt(a): out[i] =
/// {div_rn(a,b), a/b, sqrt_rn(a), sqrt(a)} (the check of gasdyn.hpp's bitwise claim)
__global__ void k_divsqrt_probe(int n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out)
{
	const int i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n) return;
	const double x = a[i], y = b[i];
	out[4*i+0] = div_rn(x, y);
	out[4*i+1] = x / y;
	out[4*i+2] = sqrt_rn(x);
	out[4*i+3] = sqrt(x);
}
void launch_divsqrt_probe(int n, const double* a, const double* b, double* out, hipStream_t s)
{ if(n > 0) k_divsqrt_probe<<<nblk(n,256), 256, 0, s>>>(n, a, b, out); }

void launch_gather_cells(const int* perm, const double* src, double* dst, int n, int width, hipStream_t s)
{ if(n > 0) k_gather<<<nblk(static_cast<long long>(n)*width,256), 256, 0, s>>>(perm, src, dst, n, width); }
void launch_scatter_cells(const int* perm, const double* src, double* dst, int n, int width, hipStream_t s)
{ if(n > 0) k_scatter<<<nblk(static_cast<long long>(n)*width,256), 256, 0, s>>>(perm, src, dst, n, width); }

}
}
