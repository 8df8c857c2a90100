/** \file blockops.hip
 * \brief The block operator on the face-based 4x4 Jacobian blocks (jacobian.hip assembles them) and every
 *   point-block preconditioner kernel on them, each factor kernel next to its solve kernel: block-Jacobi,
 *   multicolour block Gauss-Seidel, block ILU(0) in colour order and by sweeps in a row order (declarations in
 *   blockops.hpp). One thread per cell, or four lanes per cell forming one block row each (the *_rows kernels:
 *   coalesced 32-byte block rows, the same operations in the same order, so bitwise the same results).
 */
#include "blockops.hpp"
#include "blk4.hpp"

namespace fvhip {

#ifndef FVHIP_BLOCK_ROWS
#define FVHIP_BLOCK_ROWS 1
#endif

/// y = B x for a row-major fp32 4x4 block, entries widened to fp64
__device__ __forceinline__ void blk_mv(const float* __restrict__ B, const double4 x, double* y)
{
	const float4* b4 = reinterpret_cast<const float4*>(B);
	#pragma unroll
	for(int i = 0; i < 4; i++) {
		const float4 r = b4[i];
		y[i] = static_cast<double>(r.x)*x.x + static_cast<double>(r.y)*x.y + static_cast<double>(r.z)*x.z
		     + static_cast<double>(r.w)*x.w;
	}
}

// -------------------------------------------------------------------------------------------------
// y = A x with the face-based blocks; per cell: diag first, then faces in ascending reference order
// -------------------------------------------------------------------------------------------------
/// s[i] = sum_k B[i][k] x[k] for a row-major 4x4 block, rows read as double4 (k ascending)
__device__ __forceinline__ void blk_row_dots(const double* __restrict__ B, const double4 x, double (&s)[4])
{
	const double4* b4 = reinterpret_cast<const double4*>(B);
#pragma unroll
	for(int i = 0; i < 4; i++) {
		const double4 r = b4[i];
		s[i] = r.x*x.x + r.y*x.y + r.z*x.z + r.w*x.w;
	}
}
/// the same for an fp32 block (entries widened to fp64, fp64 arithmetic)
__device__ __forceinline__ void blk_row_dots(const float* __restrict__ B, const double4 x, double (&s)[4])
{
	const float4* b4 = reinterpret_cast<const float4*>(B);
#pragma unroll
	for(int i = 0; i < 4; i++) {
		const float4 r = b4[i];
		s[i] = static_cast<double>(r.x)*x.x + static_cast<double>(r.y)*x.y + static_cast<double>(r.z)*x.z
		     + static_cast<double>(r.w)*x.w;
	}
}

/// row i of a row-major 4x4 block dotted with x, as blk_row_dots forms it (k ascending)
__device__ __forceinline__ double blk_row_dot(const double* __restrict__ B, int i, const double4 x)
{
	const double4 r = reinterpret_cast<const double4*>(B)[i];
	return r.x*x.x + r.y*x.y + r.z*x.z + r.w*x.w;
}
__device__ __forceinline__ double blk_row_dot(const float* __restrict__ B, int i, const double4 x)
{
	const float4 r = reinterpret_cast<const float4*>(B)[i];
	return static_cast<double>(r.x)*x.x + static_cast<double>(r.y)*x.y + static_cast<double>(r.z)*x.z
	     + static_cast<double>(r.w)*x.w;
}

__global__ __launch_bounds__(256)
void k_block_apply(JacMesh J, const double* __restrict__ diag, const double* __restrict__ lower,
                   const double* __restrict__ upper, const double* __restrict__ x, double* __restrict__ y)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= J.ncell) return;
	const double4* x4 = reinterpret_cast<const double4*>(x);
	double acc[4];
	blk_row_dots(diag + 16*static_cast<size_t>(c), x4[c], acc);
	const int4 fc = J.cell_rfaces[c];
	const int4 nb = J.cell_nbr_fo[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface) continue;
		const double* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		double s[4];
		blk_row_dots(B, x4[nbrs[j]], s);
#pragma unroll
		for(int i = 0; i < 4; i++) acc[i] += s[i];
	}
	reinterpret_cast<double4*>(y)[c] = make_double4(acc[0], acc[1], acc[2], acc[3]);
}

/// k_block_apply with four lanes per cell, lane i forming y[c][i]: the same row dot products in the same
/// order (diagonal block first, then the faces ascending), so bitwise the same y; each block is read as four
/// consecutive 32-byte rows by four consecutive lanes, and y is written as one 32-byte row per cell
__global__ __launch_bounds__(256)
void k_block_apply_rows(JacMesh J, const double* __restrict__ diag, const double* __restrict__ lower,
                        const double* __restrict__ upper, const double* __restrict__ x, double* __restrict__ y)
{
	const long long g = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	const int c = static_cast<int>(g >> 2), i = static_cast<int>(g & 3);
	if(c >= J.ncell) return;
	const double4* x4 = reinterpret_cast<const double4*>(x);
	const int4 fc = J.cell_rfaces[c];
	const int4 nb = J.cell_nbr_fo[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
	double4 r = reinterpret_cast<const double4*>(diag + 16*static_cast<size_t>(c))[i];
	double4 xv = x4[c];
	double acc = r.x*xv.x + r.y*xv.y + r.z*xv.z + r.w*xv.w;
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface) continue;
		const double* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		r = reinterpret_cast<const double4*>(B)[i];
		xv = x4[nbrs[j]];
		acc += r.x*xv.x + r.y*xv.y + r.z*xv.z + r.w*xv.w;
	}
	y[4*static_cast<size_t>(c) + i] = acc;
}

/// t = v - A x in one pass (the multigrid's finest residuals): k_block_apply_rows' row sum, subtracted from v;
/// T = float: the blocks stored in fp32 (prec_single: the preconditioner's copy), the arithmetic in fp64
template <typename T>
__global__ __launch_bounds__(256)
void k_block_residual_rows(JacMesh J, const T* __restrict__ diag, const T* __restrict__ lower,
                           const T* __restrict__ upper, const double* __restrict__ x, const double* __restrict__ v,
                           double* __restrict__ t)
{
	const long long g = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	const int c = static_cast<int>(g >> 2), i = static_cast<int>(g & 3);
	if(c >= J.ncell) return;
	const double4* x4 = reinterpret_cast<const double4*>(x);
	const int4 fc = J.cell_rfaces[c];
	const int4 nb = J.cell_nbr_fo[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
	double acc = blk_row_dot(diag + 16*static_cast<size_t>(c), i, x4[c]);
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface) continue;
		const T* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		acc += blk_row_dot(B, i, x4[nbrs[j]]);
	}
	t[4*static_cast<size_t>(c) + i] = v[4*static_cast<size_t>(c) + i] - acc;
}

// -------------------------------------------------------------------------------------------------
// point-block Jacobi: the inverted diagonal blocks, their product, the sweeps
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_bjac_invert(int n, const double* __restrict__ diag, double* __restrict__ dinv)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= n) return;
	double a[4][4], b[4][4];
	ld16(diag + 16*static_cast<size_t>(c), a);
	inv4(a, b);
	st16(dinv + 16*static_cast<size_t>(c), b);
}

template <typename T>
__global__ __launch_bounds__(256)
void k_bjac_apply(int n, const T* __restrict__ dinv, const double* __restrict__ x, double* __restrict__ y)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= n) return;
	double o[4];
	blk_mv(dinv + 16*static_cast<size_t>(c), reinterpret_cast<const double4*>(x)[c], o);
	reinterpret_cast<double4*>(y)[c] = make_double4(o[0], o[1], o[2], o[3]);
}

/// k_bjac_apply with four lanes per cell, lane i forming y[c][i] = row i of D^-1 . x[c] (the same dot, in the
/// same order: bitwise k_bjac_apply's y), the block read as four consecutive rows by the cell's four lanes
template <typename T>
__global__ __launch_bounds__(256)
void k_bjac_apply_rows(int n, const T* __restrict__ dinv, const double* __restrict__ x, double* __restrict__ y)
{
	const long long g = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	const int c = static_cast<int>(g >> 2), i = static_cast<int>(g & 3);
	if(c >= n) return;
	const double4 xv = reinterpret_cast<const double4*>(x)[c];
	double o;
	if constexpr(sizeof(T) == sizeof(double)) {
		const double4 r = reinterpret_cast<const double4*>(dinv + 16*static_cast<size_t>(c))[i];
		o = r.x*xv.x + r.y*xv.y + r.z*xv.z + r.w*xv.w;
	} else {
		const float4 r = reinterpret_cast<const float4*>(dinv + 16*static_cast<size_t>(c))[i];
		o = static_cast<double>(r.x)*xv.x + static_cast<double>(r.y)*xv.y + static_cast<double>(r.z)*xv.z
		  + static_cast<double>(r.w)*xv.w;
	}
	y[4*static_cast<size_t>(c) + i] = o;
}

__global__ __launch_bounds__(256)
void k_bjac_correct(int n, const double* __restrict__ dinv, const double* __restrict__ b,
                    const double* __restrict__ y, double* __restrict__ z)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= n) return;
	const double4 bb = reinterpret_cast<const double4*>(b)[c], yy = reinterpret_cast<const double4*>(y)[c];
	double o[4];
	blk_mv(dinv + 16*static_cast<size_t>(c), make_double4(bb.x-yy.x, bb.y-yy.y, bb.z-yy.z, bb.w-yy.w), o);
	double4 zz = reinterpret_cast<double4*>(z)[c];
	zz.x += o[0]; zz.y += o[1]; zz.z += o[2]; zz.w += o[3];
	reinterpret_cast<double4*>(z)[c] = zz;
}

/// One block-Jacobi sweep fused into one pass: zout = D^-1 (v - sum_faces B zin[nbr]), the
/// off-diagonal half of k_block_apply followed by the diagonal solve (zin needs its ghost rows).
/// Same iterate as zin + D^-1 (v - A zin) up to rounding, without reading D or writing A zin.
template <typename T>
__global__ __launch_bounds__(256)
void k_bjac_sweep(JacMesh J, const T* __restrict__ dinv, const T* __restrict__ lower,
                  const T* __restrict__ upper, const double* __restrict__ v, const double* __restrict__ zin,
                  double* __restrict__ zout)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= J.ncell) return;
	const double4* z4 = reinterpret_cast<const double4*>(zin);
	const double4 vc = reinterpret_cast<const double4*>(v)[c];
	double acc[4] = {vc.x, vc.y, vc.z, vc.w};
	const int4 fc = J.cell_rfaces[c];
	const int4 nb = J.cell_nbr_fo[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface) continue;
		const T* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		double s[4];
		blk_row_dots(B, z4[nbrs[j]], s);
#pragma unroll
		for(int i = 0; i < 4; i++) acc[i] -= s[i];
	}
	double o[4];
	blk_row_dots(dinv + 16*static_cast<size_t>(c), make_double4(acc[0], acc[1], acc[2], acc[3]), o);
	reinterpret_cast<double4*>(zout)[c] = make_double4(o[0], o[1], o[2], o[3]);
}

/// k_bjac_sweep with four lanes per cell, lane i forming row i (coalesced block rows, as k_block_apply_rows):
/// the same row sums in the same order, the four sums exchanged within the cell's lanes for the product
/// with D^-1, so bitwise k_bjac_sweep's z
template <typename T>
__global__ __launch_bounds__(256)
void k_bjac_sweep_rows(JacMesh J, const T* __restrict__ dinv, const T* __restrict__ lower,
                       const T* __restrict__ upper, const double* __restrict__ v, const double* __restrict__ zin,
                       double* __restrict__ zout)
{
	const long long g = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	const int c = static_cast<int>(g >> 2), i = static_cast<int>(g & 3);
	const bool live = c < J.ncell;
	const int cc = live ? c : J.ncell - 1;          // lanes past the end compute a copy and store nothing
	const double4* z4 = reinterpret_cast<const double4*>(zin);
	double acc = v[4*static_cast<size_t>(cc) + i];
	const int4 fc = J.cell_rfaces[cc];
	const int4 nb = J.cell_nbr_fo[cc];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface) continue;
		const T* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		acc -= blk_row_dot(B, i, z4[nbrs[j]]);
	}
	// the cell's four row sums to every lane of the cell (all 64 lanes of the wave take part)
	const double4 t = make_double4(__shfl(acc, 0, 4), __shfl(acc, 1, 4), __shfl(acc, 2, 4), __shfl(acc, 3, 4));
	const double o = blk_row_dot(dinv + 16*static_cast<size_t>(cc), i, t);
	if(live) zout[4*static_cast<size_t>(c) + i] = o;
}

// -------------------------------------------------------------------------------------------------
// multicolour block Gauss-Seidel
// -------------------------------------------------------------------------------------------------
/// One colour of a multicolour block Gauss-Seidel sweep, in place: z_c = D^-1 (v - sum_faces B z[nbr])
/// for the listed cells, which share no face, so every neighbour value read is either from an
/// earlier colour of this sweep or from the previous sweep (ghost rows: from the last exchange).
template <typename T>
__global__ __launch_bounds__(256)
void k_bgs_colour(JacMesh J, const T* __restrict__ dinv, const T* __restrict__ lower, const T* __restrict__ upper,
                  const double* __restrict__ v, double* z, const int* __restrict__ cells, int n)
{
	const int i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n) return;
	const int c = cells[i];
	const double4* z4 = reinterpret_cast<const double4*>(z);
	const double4 vc = reinterpret_cast<const double4*>(v)[c];
	double acc[4] = {vc.x, vc.y, vc.z, vc.w};
	const int4 fc = J.cell_rfaces[c];
	const int4 nb = J.cell_nbr_fo[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface) continue;
		const T* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		double s[4];
		blk_row_dots(B, z4[nbrs[j]], s);
#pragma unroll
		for(int k = 0; k < 4; k++) acc[k] -= s[k];
	}
	double o[4];
	blk_row_dots(dinv + 16*static_cast<size_t>(c), make_double4(acc[0], acc[1], acc[2], acc[3]), o);
	reinterpret_cast<double4*>(z)[c] = make_double4(o[0], o[1], o[2], o[3]);
}

/// k_bgs_colour with four lanes per cell (k_bjac_sweep_rows' arithmetic, in place): bitwise k_bgs_colour's z.
/// Every lane of the cell reads its neighbours' rows before any lane writes the cell (cells of a colour
/// share no face, so no neighbour is written by this launch)
template <typename T>
__global__ __launch_bounds__(256)
void k_bgs_colour_rows(JacMesh J, const T* __restrict__ dinv, const T* __restrict__ lower, const T* __restrict__ upper,
                       const double* __restrict__ v, double* z, const int* __restrict__ cells, int n)
{
	const long long g = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	const int k = static_cast<int>(g >> 2), i = static_cast<int>(g & 3);
	const bool live = k < n;
	const int c = cells[live ? k : n - 1];
	const double4* z4 = reinterpret_cast<const double4*>(z);
	double acc = v[4*static_cast<size_t>(c) + i];
	const int4 fc = J.cell_rfaces[c];
	const int4 nb = J.cell_nbr_fo[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface) continue;
		const T* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		acc -= blk_row_dot(B, i, z4[nbrs[j]]);
	}
	const double4 t = make_double4(__shfl(acc, 0, 4), __shfl(acc, 1, 4), __shfl(acc, 2, 4), __shfl(acc, 3, 4));
	const double o = blk_row_dot(dinv + 16*static_cast<size_t>(c), i, t);
	if(live) z[4*static_cast<size_t>(c) + i] = o;
}

// -------------------------------------------------------------------------------------------------
// block ILU(0): the factorisation in colour order, the sweep-based factorisation and its solves
// -------------------------------------------------------------------------------------------------
/// Block ILU(0) of the operator in multicolour order (prec_ilu), the factorisation of colour q: for each
/// listed cell i
///     Dt_i = A_ii - sum_{k ~ i, colour(k) < q} A_ik Dt_k^-1 A_ki,     dinv_i = Dt_i^-1
/// over the owned neighbours across interior faces (ghost couplings are dropped: block-Jacobi across
/// ranks, as PETSc's bjacobi + ilu). The product of row i's lower factor with a neighbour's upper
/// factor lands only on the diagonal unless three cells pairwise share faces, so this D-ILU form is
/// ILU(0) itself on meshes without such triples (fvhip_colouring reports their count). Face blocks:
/// lower[fi] = A[R][L], upper[fi] = A[L][R]; rfaces code = face << 1 | cell-is-R.
__global__ __launch_bounds__(256)
void k_ilu_factor_colour(int ncell, int nbface, const int4* __restrict__ rfaces, const int4* __restrict__ nbrs,
                         const int* __restrict__ colour, int q, const double* __restrict__ diag,
                         const double* __restrict__ lower, const double* __restrict__ upper, double* dinv,
                         const int* __restrict__ cells, int n)
{
	const int t = blockIdx.x*blockDim.x + threadIdx.x;
	if(t >= n) return;
	const int c = cells[t];
	double a[4][4];
	ld16(diag + 16*static_cast<size_t>(c), a);
	const int4 fc = rfaces[c], nb = nbrs[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int ks[4] = {nb.x, nb.y, nb.z, nb.w};
	for(int j = 0; j < 4; j++) {
		const int code = codes[j], k = ks[j];
		if(code < 0 || (code >> 1) < nbface || k < 0 || k >= ncell || colour[k] >= q) continue;
		const size_t fi = static_cast<size_t>((code >> 1) - nbface);
		double aik[4][4], aki[4][4], dk[4][4], tk[4][4], p[4][4];
		ld16(((code & 1) ? lower : upper) + 16*fi, aik);
		ld16(((code & 1) ? upper : lower) + 16*fi, aki);
		ld16(dinv + 16*static_cast<size_t>(k), dk);
		mm4(dk, aki, tk);
		mm4(aik, tk, p);
		#pragma unroll
		for(int r = 0; r < 4; r++)
			#pragma unroll
			for(int s = 0; s < 4; s++) a[r][s] -= p[r][s];
	}
	double b[4][4];
	inv4(a, b);
	st16(dinv + 16*static_cast<size_t>(c), b);
}

/// One sweep of the fixed-point block ILU(0) in a row order (ilu_order, ilu_build_sweeps; the Chow-Patel
/// iteration the reference reaches through BLASTed's -blasted_async_sweeps, run synchronously): for every owned
/// cell i at once
///     dinv_out_i = (A_ii - sum_{lower k} A_ik dinv_in_k A_ki)^-1,
/// k lower if it is an owned neighbour across an interior face with rank[k] < rank[i] (rank == nullptr: the
/// internal order, k < i). Reads dinv_in, writes dinv_out (another buffer): Jacobi style, so the result does
/// not depend on the launch's schedule. k_ilu_factor_colour's arithmetic per cell
__global__ __launch_bounds__(256)
void k_ilu_sweep_factor(int ncell, int nbface, const int4* __restrict__ rfaces, const int4* __restrict__ nbrs,
                        const int* __restrict__ rank, const double* __restrict__ diag, const double* __restrict__ lower,
                        const double* __restrict__ upper, const double* __restrict__ dinv_in, double* __restrict__ dinv_out)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= ncell) return;
	double a[4][4];
	ld16(diag + 16*static_cast<size_t>(c), a);
	const int4 fc = rfaces[c], nb = nbrs[c];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int ks[4] = {nb.x, nb.y, nb.z, nb.w};
	const int rc = rank ? rank[c] : c;
	for(int j = 0; j < 4; j++) {
		const int code = codes[j], k = ks[j];
		if(code < 0 || (code >> 1) < nbface || k < 0 || k >= ncell) continue;
		if((rank ? rank[k] : k) >= rc) continue;
		const size_t fi = static_cast<size_t>((code >> 1) - nbface);
		double aik[4][4], aki[4][4], dk[4][4], tk[4][4], p[4][4];
		ld16(((code & 1) ? lower : upper) + 16*fi, aik);
		ld16(((code & 1) ? upper : lower) + 16*fi, aki);
		ld16(dinv_in + 16*static_cast<size_t>(k), dk);
		mm4(dk, aki, tk);
		mm4(aik, tk, p);
		#pragma unroll
		for(int r = 0; r < 4; r++)
			#pragma unroll
			for(int s = 0; s < 4; s++) a[r][s] -= p[r][s];
	}
	double b[4][4];
	inv4(a, b);
	st16(dinv_out + 16*static_cast<size_t>(c), b);
}

/// One sweep of a triangular solve of the sweep-based block ILU(0)/SGS (ilu_order, ilu_apply_sweeps), out of
/// place, four lanes per cell as k_bjac_sweep_rows (row dots in face-slot order, the four sums shared within
/// the cell's lanes, lanes past the end compute a copy and store nothing). Owned neighbour k of cell i is lower
/// if rank[k] < rank[i], upper if rank[k] > rank[i] (rank == nullptr: the internal order); ghost neighbours
/// are skipped (block-Jacobi across ranks).
///   UPPER = false, the forward solve of (Dt + L) y = v:    zout_i = Dt_i^-1 (w_i - sum_{lower k} A_ik zin_k),  w = v
///   UPPER = true, the backward solve of (I + Dt^-1 U) z = y:  zout_i = w_i - Dt_i^-1 sum_{upper j} A_ij zin_j,  w = y
template <typename T, bool UPPER>
__global__ __launch_bounds__(256)
void k_ilu_sweep_solve(JacMesh J, const int* __restrict__ rank, const T* __restrict__ dinv, const T* __restrict__ lower,
                       const T* __restrict__ upper, const double* __restrict__ w, const double* __restrict__ zin,
                       double* __restrict__ zout)
{
	const long long g = static_cast<long long>(blockIdx.x)*blockDim.x + threadIdx.x;
	const int c = static_cast<int>(g >> 2), i = static_cast<int>(g & 3);
	const bool live = c < J.ncell;
	const int cc = live ? c : J.ncell - 1;
	const double4* z4 = reinterpret_cast<const double4*>(zin);
	const double wi = w[4*static_cast<size_t>(cc) + i];
	double acc = UPPER ? 0.0 : wi;
	const int4 fc = J.cell_rfaces[cc];
	const int4 nb = J.cell_nbr_fo[cc];
	const int codes[4] = {fc.x, fc.y, fc.z, fc.w};
	const int nbrs[4] = {nb.x, nb.y, nb.z, nb.w};
	const int rc = rank ? rank[cc] : cc;
#pragma unroll
	for(int j = 0; j < 4; j++) {
		const int code = codes[j], k = nbrs[j];
		if(code < 0) continue;
		const int f = code >> 1;
		if(f < J.nbface || k < 0 || k >= J.ncell) continue;
		const int rk = rank ? rank[k] : k;
		if(UPPER ? rk <= rc : rk >= rc) continue;
		const T* B = ((code & 1) ? lower : upper) + 16*static_cast<size_t>(f - J.nbface);
		acc -= blk_row_dot(B, i, z4[k]);
	}
	const double4 t = make_double4(__shfl(acc, 0, 4), __shfl(acc, 1, 4), __shfl(acc, 2, 4), __shfl(acc, 3, 4));
	const double d = blk_row_dot(dinv + 16*static_cast<size_t>(cc), i, t);
	if(live) zout[4*static_cast<size_t>(c) + i] = UPPER ? wi + d : d;
}

// -------------------------------------------------------------------------------------------------
// fp32 copies of the blocks (prec_single), row-wise add
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_to_single(long long n, const double* __restrict__ a, float* __restrict__ b)
{
	const long long i = blockIdx.x*256LL + threadIdx.x;
	if(i >= n/4) return;
	const double4 v = reinterpret_cast<const double4*>(a)[i];
	reinterpret_cast<float4*>(b)[i] = make_float4(static_cast<float>(v.x), static_cast<float>(v.y),
	                                              static_cast<float>(v.z), static_cast<float>(v.w));
}

/// z += e (4 doubles per cell)
__global__ __launch_bounds__(256)
void k_add_rows(int n, const double* __restrict__ e, double* __restrict__ z)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= n) return;
	const double4 a = reinterpret_cast<const double4*>(e)[c];
	double4 b = reinterpret_cast<double4*>(z)[c];
	b.x += a.x; b.y += a.y; b.z += a.z; b.w += a.w;
	reinterpret_cast<double4*>(z)[c] = b;
}

// -------------------------------------------------------------------------------------------------
// launchers
// -------------------------------------------------------------------------------------------------
void launch_block_apply(const JacMesh& J, const double* diag, const double* lower, const double* upper,
                        const double* x, double* y, hipStream_t s)
{
	if(J.ncell <= 0) return;
	if(FVHIP_BLOCK_ROWS)
		hipLaunchKernelGGL(k_block_apply_rows, dim3(nblk(4LL*J.ncell,256)), dim3(256), 0, s, J, diag, lower, upper, x, y);
	else
		hipLaunchKernelGGL(k_block_apply, dim3(nblk(J.ncell,256)), dim3(256), 0, s, J, diag, lower, upper, x, y);
}

void launch_block_residual(const JacMesh& J, const double* diag, const double* lower, const double* upper,
                           const double* x, const double* v, double* t, hipStream_t s)
{
	if(J.ncell <= 0) return;
	hipLaunchKernelGGL(k_block_residual_rows<double>, dim3(nblk(4LL*J.ncell,256)), dim3(256), 0, s, J, diag, lower, upper, x, v, t);
}

void launch_block_residual(const JacMesh& J, const float* diag, const float* lower, const float* upper,
                           const double* x, const double* v, double* t, hipStream_t s)
{
	if(J.ncell <= 0) return;
	hipLaunchKernelGGL(k_block_residual_rows<float>, dim3(nblk(4LL*J.ncell,256)), dim3(256), 0, s, J, diag, lower, upper, x, v, t);
}

void launch_bjac_sweep(const JacMesh& J, const double* dinv, const double* lower, const double* upper,
                       const double* v, const double* zin, double* zout, hipStream_t s)
{
	if(J.ncell <= 0) return;
	if(FVHIP_BLOCK_ROWS)
		hipLaunchKernelGGL(k_bjac_sweep_rows<double>, dim3(nblk(4LL*J.ncell,256)), dim3(256), 0, s, J, dinv, lower, upper, v, zin, zout);
	else
		hipLaunchKernelGGL(k_bjac_sweep<double>, dim3(nblk(J.ncell,256)), dim3(256), 0, s, J, dinv, lower, upper, v, zin, zout);
}
void launch_bjac_sweep(const JacMesh& J, const float* dinv, const float* lower, const float* upper,
                       const double* v, const double* zin, double* zout, hipStream_t s)
{
	if(J.ncell <= 0) return;
	if(FVHIP_BLOCK_ROWS)
		hipLaunchKernelGGL(k_bjac_sweep_rows<float>, dim3(nblk(4LL*J.ncell,256)), dim3(256), 0, s, J, dinv, lower, upper, v, zin, zout);
	else
		hipLaunchKernelGGL(k_bjac_sweep<float>, dim3(nblk(J.ncell,256)), dim3(256), 0, s, J, dinv, lower, upper, v, zin, zout);
}

template <typename T>
static void launch_ilu_sweep_solve_t(const JacMesh& J, const int* rank, bool up, const T* dinv, const T* lower, const T* upper,
                                     const double* w, const double* zin, double* zout, hipStream_t s)
{
	if(J.ncell <= 0) return;
	const dim3 g(nblk(4LL*J.ncell,256)), b(256);
	if(up) hipLaunchKernelGGL((k_ilu_sweep_solve<T,true>), g, b, 0, s, J, rank, dinv, lower, upper, w, zin, zout);
	else hipLaunchKernelGGL((k_ilu_sweep_solve<T,false>), g, b, 0, s, J, rank, dinv, lower, upper, w, zin, zout);
}
void launch_ilu_sweep_solve(const JacMesh& J, const int* rank, bool up, const double* dinv, const double* lower,
                            const double* upper, const double* w, const double* zin, double* zout, hipStream_t s)
{ launch_ilu_sweep_solve_t(J, rank, up, dinv, lower, upper, w, zin, zout, s); }
void launch_ilu_sweep_solve(const JacMesh& J, const int* rank, bool up, const float* dinv, const float* lower,
                            const float* upper, const double* w, const double* zin, double* zout, hipStream_t s)
{ launch_ilu_sweep_solve_t(J, rank, up, dinv, lower, upper, w, zin, zout, s); }

template <typename T>
void launch_bgs_colour_t(const JacMesh& J, const T* dinv, const T* lower, const T* upper, const double* v,
                         double* z, const int* cells, int n, hipStream_t s)
{
	if(n <= 0) return;
	if(FVHIP_BLOCK_ROWS)
		hipLaunchKernelGGL(k_bgs_colour_rows<T>, dim3(nblk(4LL*n,256)), dim3(256), 0, s, J, dinv, lower, upper, v, z, cells, n);
	else
		hipLaunchKernelGGL(k_bgs_colour<T>, dim3(nblk(n,256)), dim3(256), 0, s, J, dinv, lower, upper, v, z, cells, n);
}
void launch_bgs_colour(const JacMesh& J, const double* dinv, const double* lower, const double* upper,
                       const double* v, double* z, const int* cells, int n, hipStream_t s)
{ launch_bgs_colour_t(J, dinv, lower, upper, v, z, cells, n, s); }
void launch_bgs_colour(const JacMesh& J, const float* dinv, const float* lower, const float* upper,
                       const double* v, double* z, const int* cells, int n, hipStream_t s)
{ launch_bgs_colour_t(J, dinv, lower, upper, v, z, cells, n, s); }

void launch_bjac_invert(int n, const double* diag, double* dinv, hipStream_t s)
{ if(n > 0) k_bjac_invert<<<nblk(n,256), 256, 0, s>>>(n, diag, dinv); }
void launch_ilu_factor_colour(int ncell, int nbface, const int4* rfaces, const int4* nbrs, const int* colour, int q,
                              const double* diag, const double* lower, const double* upper, double* dinv,
                              const int* cells, int n, hipStream_t s)
{
	if(n > 0) k_ilu_factor_colour<<<nblk(n,256), 256, 0, s>>>(ncell, nbface, rfaces, nbrs, colour, q, diag, lower, upper,
	                                                           dinv, cells, n);
}
void launch_ilu_sweep_factor(int ncell, int nbface, const int4* rfaces, const int4* nbrs, const int* rank,
                             const double* diag, const double* lower, const double* upper, const double* dinv_in,
                             double* dinv_out, hipStream_t s)
{
	if(ncell > 0) k_ilu_sweep_factor<<<nblk(ncell,256), 256, 0, s>>>(ncell, nbface, rfaces, nbrs, rank, diag, lower, upper,
	                                                                  dinv_in, dinv_out);
}

void launch_bjac_apply(int n, const double* dinv, const double* x, double* y, hipStream_t s)
{
	if(n <= 0) return;
	if(FVHIP_BLOCK_ROWS) k_bjac_apply_rows<double><<<nblk(4LL*n,256), 256, 0, s>>>(n, dinv, x, y);
	else k_bjac_apply<double><<<nblk(n,256), 256, 0, s>>>(n, dinv, x, y);
}
void launch_bjac_apply(int n, const float* dinv, const double* x, double* y, hipStream_t s)
{
	if(n <= 0) return;
	if(FVHIP_BLOCK_ROWS) k_bjac_apply_rows<float><<<nblk(4LL*n,256), 256, 0, s>>>(n, dinv, x, y);
	else k_bjac_apply<float><<<nblk(n,256), 256, 0, s>>>(n, dinv, x, y);
}
void launch_to_single(long long n, const double* a, float* b, hipStream_t s)
{ if(n > 0) k_to_single<<<nblk(n/4,256), 256, 0, s>>>(n, a, b); }
void launch_bjac_correct(int n, const double* dinv, const double* b, const double* y, double* z, hipStream_t s)
{ if(n > 0) k_bjac_correct<<<nblk(n,256), 256, 0, s>>>(n, dinv, b, y, z); }

void launch_add_rows(int n, const double* e, double* z, hipStream_t s)
{
	if(n > 0) hipLaunchKernelGGL(k_add_rows, dim3(nblk(n, 256)), dim3(256), 0, s, n, e, z);
}

}
