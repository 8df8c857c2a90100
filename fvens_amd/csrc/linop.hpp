/** \file linop.hpp
 * \brief The linear operator and preconditioner of an implicit step on one global system (system.hpp): the
 *   operator and GMRES are in implicit.cpp, the preconditioner in precond.cpp; their kernels in blockops.hip
 *   (block operator, point-block preconditioners), lines.hip (line-implicit), amg.hip and krylov.hip (vectors).
 */
#ifndef FVHIP_LINOP_HPP
#define FVHIP_LINOP_HPP

#include "system.hpp"
#include "precond_options.hpp"

#include <vector>

namespace fvhip_detail {

/// `sweeps` smoothing sweeps on level C's A_C x = b from the iterate in x (taken as 0 if `zero`). direction: 0
/// forward, 1 backward, 2 alternating from forward. smoother 0: colour Gauss-Seidel over the whole level; 1: inside
/// row blocks of `rows` rows, block-Jacobi between them -- then x is C.x or an array outside the level (copied in
/// and out), and C.x and C.x2 may have traded places afterwards (the result is in what C.x names then). precond.cpp
void smoothLevel(fvhip_ctx* h, fvhip::AmgLevel& C, int smoother, int rows, const double* b, double* x, int sweeps,
                 int direction, bool zero);

/// The linear operator and preconditioner of one implicit step
struct LinOp
{
	System& S;
	fvhip::PrecondOptions o;
	std::vector<const double*> D, Lo, Up;     ///< per handle: diagonal / lower / upper blocks
	const ArrayOf aux = [this](size_t i) { return S.hs[i]->iw.aux; };   ///< each handle's scratch vectors
	const ArrayOf t = [this](size_t i) { return S.hs[i]->iw.t; };

	/// the preconditioner's blocks of handle i in the precision it applies them in (prec_single: the fp32
	/// copies setup() made): f(PrecBlocks); the launch_* overloads select on the pointer type
	template <typename T> struct PrecBlocks { const T *diag, *dinv, *lo, *up; };
	template <typename F> void withBlocks(size_t i, F&& f) {
		const fvhip_ctx::ImplicitWork& w = S.hs[i]->iw;
		if(o.single) f(PrecBlocks<float>{w.sdiag, w.sdinv, w.slo, w.sup});
		else f(PrecBlocks<double>{D[i], w.dinv, Lo[i], Up[i]});
	}

	// the operator (implicit.cpp)
	/// y = A x with the assembled blocks; x has ghost rows, which are filled here
	void blocks(const ArrayOf& x, const ArrayOf& y);
	/// set by a precondition call asked for the norm of its output (the Arnoldi step's z), consumed by the
	/// next apply: the matrix-free operator needs |z| and the line solve summed it while writing z
	bool znorm = false;
	void apply(const ArrayOf& x, const ArrayOf& y);

	// the preconditioner (precond.cpp)
	/// the preconditioner of the current blocks: the line factorisation or the (ILU) diagonal inverses -- with
	/// the multigrid, its finest smoother -- their fp32 copies, and the multigrid's coarse operators.
	/// (PrecondOptions::check refuses prec_lines with prec_gs / prec_ilu, and the multigrid with either.)
	void setup();
	/// z = M^-1 v (z has ghost rows)
	void precondition(const ArrayOf& v, const ArrayOf& z, bool want_norm = false);
	void sweepColour(size_t i, int col, const double* v, double* z);
	void gaussSeidel(const ArrayOf& v, const ArrayOf& z), iluApply(const ArrayOf& v, const ArrayOf& z);
	void iluSweepApply(const ArrayOf& v, const ArrayOf& z), iluSweeps(const ArrayOf& v, const ArrayOf& z);
	void lineSweeps(const ArrayOf& v, const ArrayOf& z, bool want_norm), amgApply(const ArrayOf& v, const ArrayOf& z);
	void smooth0(fvhip_ctx* h, size_t i, const double* v, double* z);
	void residual0(const ArrayOf& v, const ArrayOf& z, const ArrayOf& t);
	void cycle(fvhip_ctx* h, size_t l);
};

struct GmresOut { int iters; double rnorm0, rnorm; };

}
#endif
