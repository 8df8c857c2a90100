/** \file lines.hpp
 * \brief The line-implicit preconditioner's device storage (LineSet) and launch interface (lines.hip).
 */
#ifndef FVHIP_LINES_HPP
#define FVHIP_LINES_HPP

#include <hip/hip_runtime.h>

namespace fvhip {

/// Lines of the line-implicit preconditioner (internal cell ids), sorted by length (longest first) and
/// dealt to groups of 64: lane j of group g walks line 64g + j, so one wave runs 64 recurrences side by
/// side. Everything per line cell is stored line-interleaved: row r = gstart[g] + k holds step k of the
/// group's 64 lines, slot r*64 + lane; a 4x4 block of row r is pair-interleaved, elements 2q, 2q+1 at
/// double2 index 512 r + 64 q + lane (one coalesced 16-byte load per element pair across the 64
/// lines). cell[slot] = the lane's k-th line cell or -1 once its line has ended; face[slot] (k > 0) =
/// interior face between its cells k-1 and k, fi<<1 | (cell k-1 is R); len[64 g + lane] = the lane's
/// line length (0: no line).
/// Device arrays written by the factorisation and read by the solve: D = dinvp_k (the inverted pivot
/// blocks), Lb = A[k][k-1], W = dinvp_k A[k][k+1]; G = forward-sweep scratch [rows][4][64].
struct LineSet {
	int nlines = 0, ngroups = 0;
	long long nrows = 0;             ///< rows over all groups (slots = 64 nrows)
	const int* gstart = nullptr;     ///< [ngroups+1]
	const int* cell = nullptr;       ///< [64 nrows]
	const int* face = nullptr;       ///< [64 nrows]
	const int* len = nullptr;        ///< [64 ngroups]
	int twisted_groups = 0;          ///< leading groups of 32 lines solved from both ends (lanes j, j+32)
	double *D = nullptr, *Lb = nullptr, *W = nullptr, *G = nullptr;
	double* zpart = nullptr;         ///< [ngroups] per-group sums of z.z (launch_line_solve with a norm)
	bool single = false;             ///< D, Lb, W held in fp32 (prec_single; float4 rows in the same buffers)
};
// LINE_MAX_CELLS (longest line piece) and LINE_TWIST_MIN (shortest line solved from both ends):
// precond_setup.hpp, where buildLines cuts and packs the lines
/// block-Thomas factorisation of every line (D, Lb, W of the line set) from the block operator
void launch_line_factor(const LineSet& Ls, const double* diag, const double* lower, const double* upper, hipStream_t s);
/// z = (block-tridiagonal line part of A)^-1 v; with zsq, also zsq[0] = z.z over the solved rows (each
/// lane sums the rows it writes, a fixed shuffle tree per group, a fixed-tree sum over the groups)
void launch_line_solve(const LineSet& Ls, const double* v, double* z, hipStream_t s, double* zsq = nullptr);

}
#endif
