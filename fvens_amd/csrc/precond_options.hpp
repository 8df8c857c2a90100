/** \file precond_options.hpp
 * \brief The one description of an implicit step's preconditioner (and the solver options refused with it), from
 *   a fvhip_implicit_config or a stand-alone call's arguments. Needs include/fvhip.h and the standard library only
 *   -- no device, no handle -- so it runs in CPU tests (tests/native/precond_options_check.cpp).
 */
#ifndef FVHIP_PRECOND_OPTIONS_HPP
#define FVHIP_PRECOND_OPTIONS_HPP

#include "../../include/fvhip.h"
#include <cmath>
#include <stdexcept>

namespace fvhip {

/// the threshold of a line set as a call gives it (fvhip_lines, fvhip_ctx::ensureLines)
inline void checkLineThreshold(double thr) {
	if(!(thr >= 0.0) || !std::isfinite(thr)) throw std::invalid_argument("line_threshold must be finite and >= 0 (0: 4)");
}

struct PrecondOptions
{
	/// the limits the texts of check() name; precond.cpp asserts them equal to KRY_MAXK, AMG_BLOCK_ROWS and
	/// AMG_BLOCK_ROWS_DEFAULT (krylov.hpp, which holds KRY_MAXK, and amg.hpp include the HIP runtime)
	static constexpr int RESTART_MAX = 128, BLOCK_ROWS_MAX = 2048, BLOCK_ROWS_DEFAULT = 256;

	bool matfree = false;
	bool single = false;                      ///< preconditioner blocks in fp32 (iw.sdinv/slo/sup; line factors: LineSet::single)
	bool gs = false;                          ///< multicolour block Gauss-Seidel instead of Jacobi
	bool lines = false;                       ///< line-implicit (block-tridiagonal along lines)
	bool ilu = false;                         ///< block ILU(0): in multicolour order, or (ilu_order) sweep-based in a row order
	int ilu_order = 0;                        ///< 0: colour order; 1: internal order, 2: reverse Cuthill-McKee (sweep-based)
	int ilu_build = 0, ilu_apply = 0;         ///< sweep-based form: factor sweeps (>= 0) and solve sweeps (>= 1)
	double line_thr = 0.0;                    ///< as given (0: fvhip_ctx::ensureLines' default)
	int sweeps = 1;
	int amg = 0;                              ///< aggregation multigrid levels (0: one-level preconditioner)
	int amg_sweeps = 2, amg_coarse = 6, amg_fine = 2;
	double amg_thr = 0.2;
	int amg_smoother = 0, amg_rows = BLOCK_ROWS_DEFAULT;   ///< coarse-level smoother (LinOp::cycle) and its block rows
	/// of the solver around it, refused by the same check(); a stand-alone call leaves what it does not take as it is
	int restart = 1, cgs_refine = 0;
	double min_relax = 1.0, mf_eps = 1.0;

	/// the configuration's options; the only place where its "0: the default" rules are applied (a value that
	/// check() refuses is kept as given)
	static PrecondOptions of(const fvhip_implicit_config& c) {
		PrecondOptions o;
		o.matfree = c.matrix_free != 0; o.single = c.prec_single != 0; o.gs = c.prec_gs != 0;
		o.lines = c.prec_lines != 0; o.line_thr = c.line_threshold; o.sweeps = c.prec_sweeps;
		o.ilu = c.prec_ilu != 0; o.ilu_order = c.ilu_order; o.ilu_build = c.ilu_build_sweeps; o.ilu_apply = c.ilu_apply_sweeps;
		o.amg = c.prec_amg;
		o.amg_sweeps = c.amg_sweeps == 0 ? 2 : c.amg_sweeps;
		o.amg_coarse = c.amg_coarse_sweeps == 0 ? 6 : c.amg_coarse_sweeps;
		o.amg_fine = c.amg_fine_sweeps == 0 ? o.amg_sweeps : c.amg_fine_sweeps;
		o.amg_thr = c.amg_threshold == 0.0 ? 0.2 : c.amg_threshold;
		o.amg_smoother = c.amg_smoother; o.amg_rows = c.amg_block_rows == 0 ? BLOCK_ROWS_DEFAULT : c.amg_block_rows;
		o.restart = c.restart; o.cgs_refine = c.cgs_refine; o.min_relax = c.min_relax; o.mf_eps = c.mf_eps;
		return o;
	}
	/// refuses, with the texts callers match on, every value and combination the solver does not take
	void check() const {
		auto no = [](bool bad, const char* text) { if(bad) throw std::invalid_argument(text); };
		// the sweep-based ILU's options; all zero: the colour-order ILU or none
		no(ilu_order < 0 || ilu_order > 2, "ilu_order must be 0 (colour order), 1 (internal order) or 2 (reverse Cuthill-McKee)");
		no(ilu_build < 0, "ilu_build_sweeps must be >= 0");
		no(ilu_apply < 0, "ilu_apply_sweeps must be >= 0");
		no(ilu_order == 0 && ilu_build != 0, "ilu_build_sweeps needs ilu_order 1 or 2");
		no(ilu_order == 0 && ilu_apply != 0, "ilu_apply_sweeps needs ilu_order 1 or 2");
		no(ilu_order != 0 && !ilu, "ilu_order needs prec_ilu");
		no(ilu_order != 0 && ilu_apply < 1, "ilu_apply_sweeps must be >= 1 with ilu_order 1 or 2");
		no(restart < 1 || restart > RESTART_MAX, "restart must be in [1, 128]");
		no(cgs_refine < 0 || cgs_refine > 2, "cgs_refine must be 0 (never), 1 (ifneeded) or 2 (always)");
		no(sweeps < 1, "prec_sweeps must be >= 1");
		no(amg != 0 && amg < 2, "prec_amg must be 0 (off) or >= 2 levels");
		no(amg_sweeps < 0 || amg_coarse < 0 || amg_fine < 0 || !(amg_thr >= 0.0 && amg_thr < 1.0),
		   "amg_sweeps / amg_coarse_sweeps must be >= 0 and amg_threshold in [0, 1)");
		no(amg_smoother != 0 && amg_smoother != 1, "amg_smoother must be 0 (Gauss-Seidel over the level) or 1 (block-Jacobi / Gauss-Seidel)");
		no(amg_smoother == 1 && amg == 0, "amg_smoother = 1 needs prec_amg");
		no(amg_rows < 64 || amg_rows > BLOCK_ROWS_MAX || amg_rows % 64 != 0,
		   "amg_block_rows must be 0 (the default) or a multiple of 64 in [64, 2048]");
		no(!(min_relax > 0.0), "Minimum relaxation factor is invalid!");                      // nonlinearrelaxation.cpp:20-21
		no(matfree && !(mf_eps > 0.0), "matrix-free difference step must be positive");
		no(!(line_thr >= 0.0) || !std::isfinite(line_thr), "line_threshold must be finite and >= 0 (0: the default 4)");
		no(lines && gs, "prec_lines does not combine with prec_gs");
		no(ilu && (gs || lines), "prec_ilu does not combine with prec_gs / prec_lines");
		no(amg && (gs || ilu || sweeps != 1),
		   "prec_amg combines with prec_lines and prec_single only (prec_gs / prec_ilu / prec_sweeps > 1 are one-level options)");
	}
};

/// amg_block_rows of a call (0: the default) -> the block smoother's rows per block, checked
inline int amgBlockRows(int given) {
	fvhip_implicit_config c{};
	c.restart = c.prec_sweeps = 1; c.min_relax = 1.0; c.amg_block_rows = given;
	const PrecondOptions o = PrecondOptions::of(c);
	o.check();
	return o.amg_rows;
}

}
#endif
