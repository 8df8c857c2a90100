/** \file blockops.hpp
 * \brief Launch interface of the block operator and the point-block preconditioner kernels (blockops.hip):
 *   block-Jacobi, multicolour block Gauss-Seidel, block ILU(0) in colour order and by sweeps, on the
 *   face-based 4x4 blocks of jacobian.hpp's JacMesh.
 */
#ifndef FVHIP_BLOCKOPS_HPP
#define FVHIP_BLOCKOPS_HPP

#include "jacobian.hpp"

namespace fvhip {

void launch_block_apply(const JacMesh& J, const double* diag, const double* lower, const double* upper,
                        const double* x, double* y, hipStream_t s);
/// t = v - A x (A with the ghost coupling: x needs its ghost rows), one pass
void launch_block_residual(const JacMesh& J, const double* diag, const double* lower, const double* upper,
                           const double* x, const double* v, double* t, hipStream_t s);
void launch_block_residual(const JacMesh& J, const float* diag, const float* lower, const float* upper,
                           const double* x, const double* v, double* t, hipStream_t s);

/// dinv[c] = diag[c]^-1 (Gauss-Jordan with row pivoting), c < ncell
void launch_bjac_invert(int ncell, const double* diag, double* dinv, hipStream_t s);
/// y[c] = dinv[c] x[c]
void launch_bjac_apply(int ncell, const double* dinv, const double* x, double* y, hipStream_t s);
void launch_bjac_apply(int ncell, const float* dinv, const double* x, double* y, hipStream_t s);
/// z[c] += dinv[c] (b[c] - y[c]): one block-Jacobi sweep on A z = b, given y = A z
void launch_bjac_correct(int ncell, const double* dinv, const double* b, const double* y, double* z, hipStream_t s);
/// zout = D^-1 (v - (A - D) zin): one block-Jacobi sweep (dinv: inverted diagonal blocks)
void launch_bjac_sweep(const JacMesh& J, const double* dinv, const double* lower, const double* upper,
                       const double* v, const double* zin, double* zout, hipStream_t s);
/// the same with fp32 blocks (fp64 vectors and arithmetic)
void launch_bjac_sweep(const JacMesh& J, const float* dinv, const float* lower, const float* upper,
                       const double* v, const double* zin, double* zout, hipStream_t s);

/// one colour of a multicolour block Gauss-Seidel sweep, in place on z (cells: that colour's cells)
void launch_bgs_colour(const JacMesh& J, const double* dinv, const double* lower, const double* upper,
                       const double* v, double* z, const int* cells, int n, hipStream_t s);
void launch_bgs_colour(const JacMesh& J, const float* dinv, const float* lower, const float* upper,
                       const double* v, double* z, const int* cells, int n, hipStream_t s);

/// block ILU(0) in multicolour order, colour q's rows: dinv[c] = (A_cc - sum_{earlier-colour owned
/// neighbours k} A_ck dinv[k] A_kc)^-1 for the n listed cells (k_ilu_factor_colour)
void launch_ilu_factor_colour(int ncell, int nbface, const int4* rfaces, const int4* nbrs, const int* colour, int q,
                              const double* diag, const double* lower, const double* upper, double* dinv,
                              const int* cells, int n, hipStream_t s);
/// one synchronous sweep of the fixed-point block ILU(0) in the row order `rank` (nullptr: the internal order):
/// dinv_out[i] = (A_ii - sum_{owned neighbours k, rank[k] < rank[i]} A_ik dinv_in[k] A_ki)^-1 for every owned
/// cell at once (k_ilu_sweep_factor); dinv_in and dinv_out are different buffers
void launch_ilu_sweep_factor(int ncell, int nbface, const int4* rfaces, const int4* nbrs, const int* rank,
                             const double* diag, const double* lower, const double* upper, const double* dinv_in,
                             double* dinv_out, hipStream_t s);
/// one sweep of a triangular solve of the sweep-based block ILU(0)/SGS in the row order `rank` (nullptr: the
/// internal order), out of place (k_ilu_sweep_solve): up = false, zout_i = Dt_i^-1 (w_i - sum_{lower k} A_ik
/// zin_k) with w = v; up = true, zout_i = w_i - Dt_i^-1 sum_{upper j} A_ij zin_j with w = y. dinv: the inverted
/// pivots Dt^-1. Ghost neighbours are skipped; fp32 blocks with fp64 vectors and arithmetic in the overload
void launch_ilu_sweep_solve(const JacMesh& J, const int* rank, bool up, const double* dinv, const double* lower,
                            const double* upper, const double* w, const double* zin, double* zout, hipStream_t s);
void launch_ilu_sweep_solve(const JacMesh& J, const int* rank, bool up, const float* dinv, const float* lower,
                            const float* upper, const double* w, const double* zin, double* zout, hipStream_t s);

/// b = fp32(a), n a multiple of 4
void launch_to_single(long long n, const double* a, float* b, hipStream_t s);
/// z += e over n cells
void launch_add_rows(int n, const double* e, double* z, hipStream_t s);

}
#endif
