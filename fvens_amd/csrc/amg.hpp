/** \file amg.hpp
 * \brief Aggregation multigrid preconditioner for the assembled first-order Jacobian (4x4 blocks): the
 *   device counterpart of the reference's GAMG option for the viscous NACA 0012 case
 *   (testcases/visc-naca0012/mgopts.solverc:1-35: -pc_type gamg -pc_gamg_type agg -pc_gamg_agg_nsmooths 0
 *   -pc_gamg_threshold 0.2 -pc_gamg_reuse_interpolation true -pc_mg_levels 3 -pc_mg_cycle_type v,
 *   Richardson + bjacobi/SOR smoothing with 2 iterations per level, Richardson + bjacobi/ILU coarse solve
 *   with 6 iterations).
 *
 * Setup (host, once per mesh, like -pc_gamg_reuse_interpolation): cells are aggregated along strong
 * couplings of the cell graph -- coupling of two cells = face length / centre distance, the term that
 * dominates the Jacobian blocks of thin cells (the same measure the line-implicit preconditioner uses);
 * strong when at least `threshold` times the strongest coupling of both cells -- so boundary-layer cells
 * aggregate along the wall normal (semi-coarsening). The prolongation is the tentative one (piecewise
 * constant over aggregates: -pc_gamg_agg_nsmooths 0), the coarse operators the Galerkin products
 * A_c = P^T A P, i.e. sums of fine blocks. Every coarse block's list of contributing fine blocks is built
 * on the host in ascending order, so the coarse operators are summed on the device in a fixed order:
 * deterministic, no atomics. Coarse levels are block-sparse rows (diagonal included) with a greedy
 * colouring for the multicolour block Gauss-Seidel smoother.
 *
 * Per Jacobian (each pseudo-time step): the Galerkin sums level by level and the coarse diagonal inverses.
 * Per application: one V-cycle (precond.cpp LinOp::amgApply) -- on the finest level the one-level
 * preconditioner (line-implicit or block-Jacobi) as smoother, on the coarse levels forward / backward
 * colour Gauss-Seidel, on the coarsest `coarse_sweeps` of them -- over the whole level (amg_smoother 0), or in
 * the deck's bjacobi/SOR form (amg_smoother 1, mgopts.solverc:31-32): block-Jacobi between contiguous row
 * blocks, colour Gauss-Seidel inside each, one launch per sweep (launch_amg_bjgs).
 */
#ifndef FVHIP_AMG_HPP
#define FVHIP_AMG_HPP

#include <hip/hip_runtime.h>
#include <map>
#include <vector>
#include "precond_setup.hpp"   // the host side: AmgGraph, AmgLevelHost, amgCoarsen

namespace fvhip {

/// device arrays of one coarse level
struct AmgLevel
{
	int n = 0, nnz = 0;
	const int *rowptr = nullptr, *col = nullptr, *dpos = nullptr;
	const int *cstart = nullptr, *csrc = nullptr;
	const int *mstart = nullptr, *members = nullptr, *agg = nullptr;
	const int* cells = nullptr;              ///< colour order
	const int* d_cstart_colour = nullptr;    ///< the colour starts on the device (single-workgroup sweeps)
	std::vector<int> cstart_colour;          ///< host copy of the colour starts
	int nfine = 0;                           ///< rows of the finer level
	double *val = nullptr, *dinv = nullptr;  ///< [nnz][16], [n][16]
	double *x = nullptr, *b = nullptr, *r = nullptr;   ///< [n][4]
	/// the block smoother (launch_amg_bjgs): the second iterate of its ping-pong ([n][4]; x and x2 trade places
	/// after a sweep, so the current iterate is always x), the host copy of `cells`, and per block size R the
	/// (block, colour) offsets into `cells` (amgBlockOffsets) on the host and the device, built on first use
	double* x2 = nullptr;
	std::vector<int> h_cells;
	struct BlockTable { std::vector<int> off; const int* d_off = nullptr; };
	std::map<int, BlockTable> blocks;
};

/// val[k] = sum of the listed finer-level blocks (finest: diag / lower / upper by the AmgGraph block index
/// with nfine rows and nif interior faces; else fval)
void launch_amg_galerkin_fine(const AmgLevel& L, int nfine, int nif, const double* diag, const double* lower,
                              const double* upper, hipStream_t s);
void launch_amg_galerkin(const AmgLevel& L, const double* fval, hipStream_t s);
/// dinv[i] = (diagonal block of row i)^-1
void launch_amg_invert(const AmgLevel& L, hipStream_t s);
/// b[I] = sum of r_fine over the members of aggregate I (ascending)
void launch_amg_restrict(const AmgLevel& L, const double* rfine, double* b, hipStream_t s);
/// x_fine[i] += x[agg[i]]
void launch_amg_prolong(const AmgLevel& L, const double* x, double* xfine, hipStream_t s);
/// r = b - A x on a coarse level
void launch_amg_residual(const AmgLevel& L, const double* x, const double* b, double* r, hipStream_t s);
/// one colour of a block Gauss-Seidel sweep on A x = b, in place: x_i = dinv_i (b_i - sum_{j != i} A_ij x_j)
void launch_amg_gs_colour(const AmgLevel& L, int q, const double* b, double* x, hipStream_t s);
/// levels of at most AMG_BLOCK_ROWS rows: `sweeps` whole Gauss-Seidel sweeps (colours forward on even sweeps,
/// backward on odd ones when `alternate`, else all in direction `fwd`) in one workgroup, a barrier between
/// colours -- the same row updates in the same order as per-colour launches, without a launch per colour;
/// zero: x = 0 first. The iterate is held in LDS (32 B a row: 64 KB at the limit)
constexpr int AMG_BLOCK_ROWS = 2048;
void launch_amg_gs_block(const AmgLevel& L, const double* b, double* x, int sweeps, bool fwd, bool alternate,
                         bool zero, hipStream_t s);
constexpr int AMG_BLOCK_ROWS_DEFAULT = 256;   ///< fvhip_implicit_config::amg_block_rows = 0
/// one sweep xout = S(xin) of block-Jacobi between contiguous row blocks of R rows (block k = rows [kR, min(n,
/// (k+1)R)), R a multiple of 64 in [64, AMG_BLOCK_ROWS]) with colour Gauss-Seidel inside each block, a level of
/// any size in one launch: one workgroup per block holds its rows in LDS (32 R bytes), walks the colours in
/// direction `fwd` with a barrier after each, and reads columns outside its block from xin, which no workgroup
/// writes (xin != xout). The row update and its summation order are those of launch_amg_gs_colour. zero: xin is
/// taken as 0 and not read. d_off: amgBlockOffsets(.., R) on the device
void launch_amg_bjgs(const AmgLevel& L, int R, const int* d_off, const double* b, const double* xin, double* xout,
                     bool fwd, bool zero, hipStream_t s);

}
#endif
