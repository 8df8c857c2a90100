/** \file precond.cpp
 * \brief The preconditioner of the implicit step: the handle's structures and factors, LinOp::setup and
 *   LinOp::precondition with all they call, the multigrid's level smoother, and the entry points that apply or
 *   inspect a preconditioner on its own.
 */
#include "linop.hpp"

#include <cmath>
#include <vector>

static_assert(PrecondOptions::RESTART_MAX == KRY_MAXK && PrecondOptions::BLOCK_ROWS_MAX == AMG_BLOCK_ROWS
              && PrecondOptions::BLOCK_ROWS_DEFAULT == AMG_BLOCK_ROWS_DEFAULT, "precond_options.hpp restates these limits");

// --- the preconditioners' structures on the device: built on the host (precond_setup.hpp), uploaded here ---

void fvhip_ctx::ensureColouring() {
	if(d_gs_cells) return;
	Colouring C = colourCells(cellGraph(L));
	d_gs_cells = upload(C.cells, owned);
	d_gs_colour = upload(C.colour, owned);
	gs_triples = C.triples;
	gs_colour_start = std::move(C.colour_start);
	gs_colour = std::move(C.colour);
}

const fvhip_ctx::IluRowOrder& fvhip_ctx::ensureIluOrder(int order) {
	if(order != 1 && order != 2) throw std::invalid_argument("ilu_order must be 1 (internal order) or 2 (reverse Cuthill-McKee)");
	IluRowOrder& O = ilu_orders[order];
	if(O.built) return O;
	IluOrder H = iluOrder(cellGraph(L), order);
	if(order == 2 && L.ncell > 0) O.d_rank = upload(H.rank, owned);
	O.rank = std::move(H.rank);
	O.depth = H.depth;
	O.built = true;
	return O;
}

void fvhip_ctx::ensureLines(double thr) {
	checkLineThreshold(thr);
	if(thr == 0.0) thr = 4.0;
	if(lines.gstart && lines_thr == thr) return;
	// a rebuild (another threshold) releases the previous line set's device arrays
	for(const void* p : std::initializer_list<const void*>{lines.gstart, lines.cell, lines.face, lines.len, lines.D,
	                                                       lines.Lb, lines.W, lines.G, lines.zpart}) release(p);
	lines = LineSet{};
	LinePlan P = buildLines(cellGraph(L), thr);
	lines.twisted_groups = P.twisted_groups; lines.nlines = P.nlines; lines.ngroups = P.ngroups; lines.nrows = P.nrows;
	lines.gstart = upload(P.gstart, owned); lines.cell = upload(P.cell, owned);
	lines.face = upload(P.face, owned); lines.len = upload(P.len, owned);
	h_line_start = std::move(P.line_start); h_line_cells = std::move(P.line_cells); h_line_faces = std::move(P.line_faces);
	const size_t rows = std::max<size_t>(static_cast<size_t>(P.nrows), 1);
	lines.D = dalloc(1024*rows, owned);
	// zeroed once: in a twisted group the factorisation writes the twist row of D for lane j only
	// (the pivot); k_line_solve's forward prefetch also requests that row for lane j+32 and discards
	// it, so it must hold defined values, never garbage a later change could start using
	HC(hipMemsetAsync(lines.D, 0, sizeof(double)*1024*rows, stream));
	lines.Lb = dalloc(1024*rows, owned); lines.W = dalloc(1024*rows, owned); lines.G = dalloc(256*rows, owned);
	lines.zpart = dalloc(static_cast<size_t>(std::max(P.ngroups, 1)), owned);
	lines_thr = thr;
}

/// levels >= 2 and thr in [0, 1): every caller has checked them (PrecondOptions::check, applyAmg)
void fvhip_ctx::ensureAmg(int levels, double thr) {
	if(amg_levels == levels && amg_thr == thr) return;
	if(!amg.empty()) throw std::runtime_error("prec_amg: the hierarchy is built once per handle (same levels and threshold)");
	AmgGraph g = amgFineGraph(cellGraph(L));
	for(int l = 1; l < levels; l++) {
		if(g.n < 64) break;
		AmgLevelHost H = amgCoarsen(g, thr);
		if(H.n*5 > g.n*4) break;                         // shrinks by less than 1.25: stop
		AmgLevel D;
		D.n = H.n; D.nnz = H.rowptr[H.n]; D.nfine = g.n;
		D.rowptr = upload(H.rowptr, owned); D.col = upload(H.col, owned); D.dpos = upload(H.dpos, owned);
		D.cstart = upload(H.cstart, owned); D.csrc = upload(H.csrc, owned);
		D.mstart = upload(H.mstart, owned); D.members = upload(H.members, owned); D.agg = upload(H.agg, owned);
		D.cells = upload(H.cells, owned); D.cstart_colour = H.cstart_colour;
		D.d_cstart_colour = upload(H.cstart_colour, owned);
		D.val = dalloc(16*static_cast<size_t>(D.nnz), owned); D.dinv = dalloc(16*static_cast<size_t>(D.n), owned);
		D.x = dalloc(4*static_cast<size_t>(D.n), owned); D.b = dalloc(4*static_cast<size_t>(D.n), owned);
		D.r = dalloc(4*static_cast<size_t>(D.n), owned);
		D.x2 = dalloc(4*static_cast<size_t>(D.n), owned); D.h_cells = H.cells;
		amg.push_back(D);
		g = amgGraphOf(H);
	}
	if(amg.empty()) throw std::runtime_error("prec_amg: the mesh does not coarsen");
	amg_levels = levels;
	amg_thr = thr;
}

// --- the factors of the current blocks ---

void fvhip_ctx::iluFactor(const double* diag, const double* lower, const double* upper, double* dinv, hipStream_t st) {
	if(!st) st = stream;
	ensureColouring();
	const int nc = static_cast<int>(gs_colour_start.size()) - 1;
	timed_on(st, "k_ilu_factor", [&]{
		for(int q = 0; q < nc; q++) {
			const int b = gs_colour_start[q], n = gs_colour_start[q+1] - b;
			launch_ilu_factor_colour(L.ncell, L.nbface, J.cell_rfaces, J.cell_nbr_fo, d_gs_colour, q, diag, lower, upper,
			                         dinv, d_gs_cells + b, n, st);
		}
	});
}

void fvhip_ctx::iluSweepFactor(int order, int build, const double* diag, const double* lower, const double* upper, double* dinv) {
	const IluRowOrder& O = ensureIluOrder(order);
	const size_t N = static_cast<size_t>(L.ncell);
	if(!ilu_dinv2) { ilu_dinv2 = dalloc(16*N, owned); ilu_p = dalloc(4*N, owned); ilu_q = dalloc(4*N, owned); }
	auto buf = [&](int s) { return (build - s) % 2 == 0 ? dinv : ilu_dinv2; };
	timed("k_bjac_invert", [&]{ launch_bjac_invert(L.ncell, diag, buf(0), stream); });
	for(int s = 1; s <= build; s++)
		timed("k_ilu_sweep_factor", [&]{
			launch_ilu_sweep_factor(L.ncell, L.nbface, J.cell_rfaces, J.cell_nbr_fo, O.d_rank, diag, lower, upper,
			                        buf(s - 1), buf(s), stream);
		});
}

const int* fvhip_ctx::amgBlocks(AmgLevel& C, int R) {
	AmgLevel::BlockTable& T = C.blocks[R];
	if(!T.d_off) {
		T.off = amgBlockOffsets(C.n, C.cstart_colour, C.h_cells, R);
		T.d_off = upload(T.off, owned);
	}
	return T.d_off;
}

void fvhip_ctx::amgSetup(const double* diag, const double* lower, const double* upper) {
	timed("k_amg_galerkin", [&]{
		for(size_t l = 0; l < amg.size(); l++) {
			if(l == 0) launch_amg_galerkin_fine(amg[0], L.ncell, L.ninface, diag, lower, upper, stream);
			else launch_amg_galerkin(amg[l], amg[l-1].val, stream);
			launch_amg_invert(amg[l], stream);
		}
	});
}

void fvhip_ctx::ensureSinglePrecond() {
	if(iw.sdinv) return;
	const size_t N = static_cast<size_t>(L.ncell);
	const size_t Fi = static_cast<size_t>(std::max(L.ninface, 1));
	iw.sdinv = reinterpret_cast<float*>(dalloc(8*N, owned));
	iw.slo = reinterpret_cast<float*>(dalloc(8*Fi, owned));
	iw.sup = reinterpret_cast<float*>(dalloc(8*Fi, owned));
	iw.sdiag = reinterpret_cast<float*>(dalloc(8*N, owned));
}

namespace fvhip_detail {

/// `sweeps` sweeps of the block smoother (launch_amg_bjgs, blocks of R rows) on A_C x = b, the iterate in C.x
/// (taken as 0 if `zero`): each sweep reads C.x and writes C.x2, which then trade places, so the result is in
/// C.x again; from zero the first sweep reads no iterate and writes C.x itself
static void amgBlockSweeps(fvhip_ctx* h, AmgLevel& C, int R, const double* b, int sweeps, int direction, bool zero)
{
	const int* off = h->amgBlocks(C, R);
	if(zero && sweeps < 1) exact::launch_fill(C.x, 0.0, 4LL*C.n, h->stream);
	for(int k = 0; k < sweeps; k++) {
		const bool fwd = direction == 2 ? k % 2 == 0 : direction == 0;
		if(zero && k == 0) { launch_amg_bjgs(C, R, off, b, C.x2, C.x, fwd, true, h->stream); continue; }
		launch_amg_bjgs(C, R, off, b, C.x, C.x2, fwd, false, h->stream);
		std::swap(C.x, C.x2);
	}
}

void smoothLevel(fvhip_ctx* h, AmgLevel& C, int smoother, int rows, const double* b, double* x, int sweeps,
                 int direction, bool zero)
{
	if(smoother == 1) {              // block-Jacobi / Gauss-Seidel: one launch per sweep on a level of any size
		const bool outside = x != C.x;
		const size_t bytes = 4*sizeof(double)*static_cast<size_t>(C.n);
		if(outside && !zero) HC(hipMemcpyAsync(C.x, x, bytes, hipMemcpyDeviceToDevice, h->stream));
		amgBlockSweeps(h, C, rows, b, sweeps, direction, zero);
		if(outside) HC(hipMemcpyAsync(x, C.x, bytes, hipMemcpyDeviceToDevice, h->stream));
	} else if(C.n <= AMG_BLOCK_ROWS) {   // one workgroup sweeps the level (no launch per colour)
		launch_amg_gs_block(C, b, x, sweeps, direction != 1, direction == 2, zero, h->stream);
	} else {
		if(zero) exact::launch_fill(x, 0.0, 4LL*C.n, h->stream);
		const int nc = static_cast<int>(C.cstart_colour.size()) - 1;
		for(int k = 0; k < sweeps; k++) {
			const bool fwd = direction == 2 ? k % 2 == 0 : direction == 0;
			for(int q = 0; q < nc; q++) launch_amg_gs_colour(C, fwd ? q : nc - 1 - q, b, x, h->stream);
		}
	}
}

/// z = M^-1 v: by default `sweeps` block-Jacobi sweeps on A z = v from z = 0. The iterates alternate between z and
/// aux (both with ghost rows) so that the last one lands in z.
void LinOp::precondition(const ArrayOf& v, const ArrayOf& z, bool want_norm) {
	znorm = false;
	if(o.amg) { amgApply(v, z); return; }
	if(o.gs) { gaussSeidel(v, z); return; }
	if(o.lines) { lineSweeps(v, z, want_norm); return; }
	if(o.ilu) { iluSweeps(v, z); return; }
	auto buf = [&](int k) -> const ArrayOf& { return ((o.sweeps - 1 - k) % 2 == 0) ? z : aux; };
	S.each([&](size_t i, fvhip_ctx* h) {
		h->timed("k_bjac_apply", [&]{
			withBlocks(i, [&](auto B) { launch_bjac_apply(h->L.ncell, B.dinv, v(i), buf(0)(i), h->stream); });
		});
	});
	for(int k = 1; k < o.sweeps; k++) {
		const ArrayOf& zin = buf(k-1);
		const ArrayOf& zout = buf(k);
		S.exchange(zin, 4);
		S.each([&](size_t i, fvhip_ctx* h) {
			h->timed("k_bjac_sweep", [&]{
				withBlocks(i, [&](auto B) { launch_bjac_sweep(h->J, B.dinv, B.lo, B.up, v(i), zin(i), zout(i), h->stream); });
			});
		});
	}
}
/// colour `col` of handle i's block Gauss-Seidel sweep on A z = v, in place on z
void LinOp::sweepColour(size_t i, int col, const double* v, double* z) {
	fvhip_ctx* h = S.hs[i];
	const int b = h->gs_colour_start[col], n = h->gs_colour_start[col+1] - b;
	withBlocks(i, [&](auto B) { launch_bgs_colour(h->J, B.dinv, B.lo, B.up, v, z, h->d_gs_cells + b, n, h->stream); });
}
/// z = M^-1 v by `sweeps` multicolour block Gauss-Seidel sweeps from z = 0, colours in forward
/// then backward order on alternate sweeps (symmetric Gauss-Seidel pairs). Across ranks the
/// sweep is block-Jacobi: ghost rows are exchanged once per sweep -- the reference's PETSc
/// setting -pc_type bjacobi -sub_pc_type sor, with a colour order instead of a row order.
void LinOp::gaussSeidel(const ArrayOf& v, const ArrayOf& z) {
	S.each([&](size_t i, fvhip_ctx* h) {
		exact::launch_fill(z(i), 0.0, 4LL*(h->L.ncell + h->L.nghost), h->stream);
	});
	for(int k = 0; k < o.sweeps; k++) {
		if(k > 0) S.exchange(z, 4);
		const bool fwd = (k % 2) == 0;
		S.each([&](size_t i, fvhip_ctx* h) {
			const int nc = static_cast<int>(h->gs_colour_start.size()) - 1;
			h->timed("k_bgs_colour", [&]{
				for(int q = 0; q < nc; q++) sweepColour(i, fwd ? q : nc - 1 - q, v(i), z(i));
			});
		});
	}
}
/// z = M^-1 v for the block ILU(0) M = (Dt + L) Dt^-1 (Dt + U) in colour order: a forward pass over
/// the colours from z = 0 gives y = (Dt + L)^-1 v, the backward pass z_i = Dt_i^-1 (v_i - sum_{earlier}
/// A_ik y_k - sum_{later} A_ij z_j) = y_i - Dt_i^-1 sum_{later} A_ij z_j -- both are the Gauss-Seidel
/// colour kernel with the ILU pivots. Ghost rows stay zero (no exchange: block-Jacobi across ranks)
void LinOp::iluApply(const ArrayOf& v, const ArrayOf& z) {
	if(o.ilu_order) { iluSweepApply(v, z); return; }
	S.each([&](size_t i, fvhip_ctx* h) {
		exact::launch_fill(z(i), 0.0, 4LL*(h->L.ncell + h->L.nghost), h->stream);
		const int nc = static_cast<int>(h->gs_colour_start.size()) - 1;
		h->timed("k_ilu_solve", [&]{
			// forward over colours 0..nc-1, backward over nc-2..0: the last colour's backward value
			// would be its forward one again (all its neighbours are of earlier colours)
			for(int q = 0; q < 2*nc - 1; q++) sweepColour(i, q < nc ? q : 2*nc - 2 - q, v(i), z(i));
		});
	});
}
/// z = M^-1 v for the sweep-based block ILU(0)/SGS in a row order (ilu_order; the reference's BLASTed
/// -blasted_async_sweeps b,a with init_zero, run synchronously): a = ilu_apply Jacobi-style sweeps on each
/// triangular system from a zero guess,
///     y^1 = Dt^-1 v,  y^{m+1}_i = Dt_i^-1 (v_i - sum_{lower k} A_ik y^m_k),      y = y^a,
///     z^1 = y,        z^{m+1}_i = y_i - Dt_i^-1 sum_{upper j} A_ij z^m_j,        z = z^a,
/// a forward and a - 1 backward launches over all cells, each out of place. The forward iterates alternate
/// between z and the handle's ilu_p so that y lands in ilu_p (in z if a = 1), the backward ones between z and
/// ilu_q so that the last lands in z. A fixed linear operator of v (exact once a reaches the order's depth).
/// Ghost neighbours are skipped and ghost rows of z are not written: block-Jacobi across ranks
void LinOp::iluSweepApply(const ArrayOf& v, const ArrayOf& z) {
	const int a = o.ilu_apply;
	S.each([&](size_t i, fvhip_ctx* h) {
		const int* rank = h->ensureIluOrder(o.ilu_order).d_rank;
		double *p = h->ilu_p, *q = h->ilu_q, *zi = z(i);
		auto fwd = [&](int m) { return a == 1 || (a - m) % 2 != 0 ? zi : p; };          // y^m, m = 1 .. a
		auto bwd = [&](int m) { return m == 1 ? p : (a - m) % 2 == 0 ? zi : q; };        // z^m, m = 1 .. a
		withBlocks(i, [&](auto B) {
			h->timed("k_bjac_apply", [&]{ launch_bjac_apply(h->L.ncell, B.dinv, v(i), fwd(1), h->stream); });
			for(int m = 2; m <= a; m++)
				h->timed("k_ilu_sweep_solve", [&]{
					launch_ilu_sweep_solve(h->J, rank, false, B.dinv, B.lo, B.up, v(i), fwd(m - 1), fwd(m), h->stream);
				});
			for(int m = 2; m <= a; m++)
				h->timed("k_ilu_sweep_solve", [&]{
					launch_ilu_sweep_solve(h->J, rank, true, B.dinv, B.lo, B.up, p, bwd(m - 1), bwd(m), h->stream);
				});
		});
	});
}
/// ILU(0), then `sweeps` - 1 corrections z += M^-1 (v - A z) (A with the ghost coupling)
void LinOp::iluSweeps(const ArrayOf& v, const ArrayOf& z) {
	iluApply(v, z);
	for(int k = 1; k < o.sweeps; k++) {
		blocks(z, t);
		S.each([&](size_t i, fvhip_ctx* h) { launch_axpby(4LL*h->L.ncell, 1.0, v(i), -1.0, t(i), h->stream); });
		iluApply(t, aux);
		S.each([&](size_t i, fvhip_ctx* h) { launch_add_rows(h->L.ncell, aux(i), z(i), h->stream); });
	}
}
/// z = M^-1 v with M the block-tridiagonal line part of A (factorised in setup), then `sweeps` - 1
/// corrections z += M^-1 (v - A z) (A with the ghost coupling: block-Jacobi across ranks)
void LinOp::lineSweeps(const ArrayOf& v, const ArrayOf& z, bool want_norm) {
	// one sweep on one domain for the matrix-free operator: the line solve also returns |z|^2
	const bool norm = want_norm && o.matfree && o.sweeps == 1 && S.size() == 1 && !S.legs && !S.halo();
	S.each([&](size_t i, fvhip_ctx* h) {
		h->timed("k_line_solve", [&]{ launch_line_solve(h->lines, v(i), z(i), h->stream, norm ? h->iw.red : nullptr); });
	});
	znorm = norm;
	for(int k = 1; k < o.sweeps; k++) {
		blocks(z, t);
		S.each([&](size_t i, fvhip_ctx* h) {
			launch_axpby(4LL*h->L.ncell, 1.0, v(i), -1.0, t(i), h->stream);
			h->timed("k_line_solve", [&]{ launch_line_solve(h->lines, t(i), aux(i), h->stream); });
			launch_add_rows(h->L.ncell, aux(i), z(i), h->stream);
		});
	}
}
/// z = the finest smoother applied to v (line solve, else D^-1 v)
void LinOp::smooth0(fvhip_ctx* h, size_t i, const double* v, double* z) {
	if(o.lines) h->timed("k_line_solve", [&]{ launch_line_solve(h->lines, v, z, h->stream); });
	else withBlocks(i, [&](auto B) { launch_bjac_apply(h->L.ncell, B.dinv, v, z, h->stream); });
}
/// t = v - A z (A with the ghost coupling)
void LinOp::residual0(const ArrayOf& v, const ArrayOf& z, const ArrayOf& t) {
	S.exchange(z, 4);
	S.each([&](size_t i, fvhip_ctx* h) {
		h->timed("k_block_residual", [&]{
			withBlocks(i, [&](auto B) { launch_block_residual(h->J, B.diag, B.lo, B.up, z(i), v(i), t(i), h->stream); });
		});
	});
}
/// coarse level l of handle h's hierarchy: V-cycle on A_l x_l = b_l from x_l = 0 (forward sweeps before the
/// coarse correction, backward after it; the coarsest level amg_coarse sweeps, alternating). amg_smoother 0:
/// Gauss-Seidel over the whole level; 1: inside row blocks of amg_rows rows, block-Jacobi between them
/// (mgopts.solverc:31-32), same sweep counts and directions
void LinOp::cycle(fvhip_ctx* h, size_t l) {
	AmgLevel& C = h->amg[l];
	auto smooth = [&](int sweeps, int direction, bool zero) {
		smoothLevel(h, C, o.amg_smoother, o.amg_rows, C.b, C.x, sweeps, direction, zero);
	};
	if(l + 1 == h->amg.size()) { smooth(o.amg_coarse, 2, true); return; }
	smooth(o.amg_sweeps, 0, true);
	launch_amg_residual(C, C.x, C.b, C.r, h->stream);
	AmgLevel& F = h->amg[l+1];
	launch_amg_restrict(F, C.r, F.b, h->stream);
	cycle(h, l + 1);
	launch_amg_prolong(F, F.x, C.x, h->stream);
	smooth(o.amg_sweeps, 1, false);
}
/// z = M^-1 v, M one V-cycle of the aggregation multigrid (block-Jacobi across ranks: each handle's hierarchy
/// covers its owned cells; the finest residuals include the ghost coupling)
void LinOp::amgApply(const ArrayOf& v, const ArrayOf& z) {
	S.each([&](size_t i, fvhip_ctx* h) { smooth0(h, i, v(i), z(i)); });
	auto correct = [&]() {             // z += M0^-1 (v - A z)
		residual0(v, z, t);
		S.each([&](size_t i, fvhip_ctx* h) { smooth0(h, i, t(i), aux(i)); launch_add_rows(h->L.ncell, aux(i), z(i), h->stream); });
	};
	for(int k = 1; k < o.amg_fine; k++) correct();
	residual0(v, z, t);
	S.each([&](size_t i, fvhip_ctx* h) {
		h->timed("k_amg_cycle", [&]{
			launch_amg_restrict(h->amg[0], t(i), h->amg[0].b, h->stream);
			cycle(h, 0);
			launch_amg_prolong(h->amg[0], h->amg[0].x, z(i), h->stream);
		});
	});
	for(int k = 0; k < o.amg_fine; k++) correct();
}
void LinOp::setup() {
	S.each([&](size_t i, fvhip_ctx* h) {
		const fvhip_ctx::ImplicitWork& w = h->iw;
		if(o.lines) {
			h->ensureLines(o.line_thr);
			h->lines.single = o.single;
			h->timed("k_line_factor", [&]{ launch_line_factor(h->lines, D[i], Lo[i], Up[i], h->stream); });
		} else if(o.ilu && o.ilu_order) h->iluSweepFactor(o.ilu_order, o.ilu_build, D[i], Lo[i], Up[i], w.dinv);
		else if(o.ilu) h->iluFactor(D[i], Lo[i], Up[i], w.dinv);
		else h->timed("k_bjac_invert", [&]{ launch_bjac_invert(h->L.ncell, D[i], w.dinv, h->stream); });
		if(o.gs) h->ensureColouring();
		if(o.single && (o.amg || !o.lines)) {      // (the line factors are stored in fp32 by the factorisation itself)
			h->ensureSinglePrecond();
			const long long nd = 16LL*h->L.ncell, nf = 16LL*std::max(h->L.ninface, 0);
			auto convert = [&](long long n, const double* a, float* b) { launch_to_single(n, a, b, h->stream); };
			h->timed("k_to_single", [&]{
				if(o.amg) convert(nd, D[i], w.sdiag);      // the finest operator, for the smoother's residuals
				else convert(nd, w.dinv, w.sdinv);
				if(o.amg || o.sweeps > 1 || o.gs || o.ilu) { convert(nf, Lo[i], w.slo); convert(nf, Up[i], w.sup); }
				if(o.amg && !o.lines) convert(nd, w.dinv, w.sdinv);
			});
		}
		if(o.amg) {
			h->ensureAmg(o.amg, o.amg_thr);
			h->amgSetup(D[i], Lo[i], Up[i]);
		}
	});
}

/// one coarse level of a handle by its number from 1 (the first coarse level)
static AmgLevel& amgLevelOf(fvhip_handle h, int level)
{
	need(h, "handle");
	if(level < 1 || level > static_cast<int>(h->amg.size())) throw std::invalid_argument("no such multigrid level");
	return h->amg[static_cast<size_t>(level) - 1];
}

/// the stricter rules of the two stand-alone multigrid calls, before they look at their handles
static void checkAmgCall(int levels, int sweeps, int coarse_sweeps, const void* d_v, const void* d_z)
{
	if(levels < 2 || sweeps < 1 || coarse_sweeps < 1) throw std::invalid_argument("levels >= 2, sweeps >= 1, coarse_sweeps >= 1");
	if((d_v == nullptr) != (d_z == nullptr)) throw std::invalid_argument("v and z go together");
}
static int checkAmgSmoother(int smoother, int block_rows)
{
	if(smoother != 0 && smoother != 1) throw std::invalid_argument("smoother must be 0 or 1");
	return amgBlockRows(block_rows);
}

/// the body of the two stand-alone multigrid calls: sets the multigrid up on the given blocks of every handle and,
/// with v, applies one V-cycle
static void applyAmg(System& S, const double* const* d_diag, const double* const* d_lower, const double* const* d_upper,
                     int levels, double threshold, int sweeps, int coarse_sweeps, double line_threshold,
                     const double* const* d_v, double* const* d_z, int smoother, int rows)
{
	S.each([&](size_t, fvhip_ctx* h) { h->ensureImplicit(1); });
	LinOp A{S};
	A.o.amg = levels; A.o.amg_sweeps = A.o.amg_fine = sweeps; A.o.amg_coarse = coarse_sweeps; A.o.amg_thr = threshold;
	A.o.amg_smoother = smoother; A.o.amg_rows = rows;
	A.o.lines = line_threshold > 0.0; A.o.line_thr = A.o.lines ? line_threshold : 0.0;
	// the call's own thresholds are no configuration fields and keep their texts
	checkLineThreshold(A.o.line_thr);
	if(!(threshold >= 0.0 && threshold < 1.0)) throw std::invalid_argument("amg_threshold must be in [0, 1)");
	A.o.check();
	const size_t n = S.size();
	A.D.assign(d_diag, d_diag + n); A.Lo.assign(d_lower, d_lower + n); A.Up.assign(d_upper, d_upper + n);
	A.setup();
	if(d_v) {
		// z needs ghost rows for the finest residuals: each handle's own operand buffer
		A.precondition([&](size_t i) { return const_cast<double*>(d_v[i]); }, [&](size_t i) { return S.hs[i]->iw.z; });
		S.each([&](size_t i, fvhip_ctx* h) {
			HC(hipMemcpyAsync(d_z[i], h->iw.z, 4*sizeof(double)*static_cast<size_t>(h->L.ncell), hipMemcpyDeviceToDevice, h->stream));
		});
	}
	S.each([&](size_t, fvhip_ctx*) { HC(hipGetLastError()); });
	S.sync();
}

}

using namespace fvhip_detail;

extern "C" {

int fvhip_line_precondition_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                   double line_threshold, int single, const double* d_v, double* d_z)
{
	return guard([&] {
		need(h, "handle");
		needBlocks(h->L.ninface, d_diag, d_lower, d_upper); need(d_v, "v"); need(d_z, "z");
		HC(hipSetDevice(h->device));
		h->ensureLines(line_threshold);
		h->lines.single = single != 0;
		launch_line_factor(h->lines, d_diag, d_lower, d_upper, h->stream);
		launch_line_solve(h->lines, d_v, d_z, h->stream);
		HC(hipGetLastError());
		HC(hipStreamSynchronize(h->stream));
	});
}

/// z = M^-1 v on one handle with the preconditioner `o` of the given blocks
static void applyOnce(System& S, const PrecondOptions& o, const double* d_diag, const double* d_lower, const double* d_upper,
                      const double* d_v, double* d_z)
{
	S.hs[0]->ensureImplicit(1);
	LinOp A{S, o};
	A.D = {d_diag}; A.Lo = {d_lower}; A.Up = {d_upper};
	A.setup();
	A.precondition([&](size_t) { return const_cast<double*>(d_v); }, [&](size_t) { return d_z; });
	HC(hipGetLastError());
	S.sync();
}

int fvhip_ilu_precondition_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                  const double* d_v, double* d_z)
{
	return guard([&] {
		need(h, "handle");
		needBlocks(h->L.ninface, d_diag, d_lower, d_upper); need(d_v, "v"); need(d_z, "z");
		PrecondOptions o;
		o.ilu = true;
		o.check();
		System S = single(h);
		applyOnce(S, o, d_diag, d_lower, d_upper, d_v, d_z);
	});
}

int fvhip_ilu_sweeps_precondition_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                         int order, int build_sweeps, int apply_sweeps, int single, const double* d_v,
                                         double* d_z)
{
	return guard([&] {
		need(h, "handle");
		needBlocks(h->L.ninface, d_diag, d_lower, d_upper); need(d_v, "v"); need(d_z, "z");
		PrecondOptions o;
		o.ilu = true; o.single = single != 0;
		o.ilu_order = order; o.ilu_build = build_sweeps; o.ilu_apply = apply_sweeps;
		o.check();
		if(order == 0) throw std::invalid_argument("ilu_order must be 1 (internal order) or 2 (reverse Cuthill-McKee)");
		// ghost rows are neither read nor written (block-Jacobi across ranks), so a rank's handle needs neither its
		// communicator nor its group here
		System S{{h}, {}};
		HC(hipSetDevice(h->device));
		applyOnce(S, o, d_diag, d_lower, d_upper, d_v, d_z);
	});
}

int fvhip_ilu_order(fvhip_handle h, int order, int* rank, int* depth)
{
	return guard([&] {
		need(h, "handle");
		HC(hipSetDevice(h->device));
		const fvhip_ctx::IluRowOrder& O = h->ensureIluOrder(order);
		if(rank) std::copy(O.rank.begin(), O.rank.end(), rank);
		if(depth) *depth = O.depth;
	});
}

int fvhip_amg_precondition_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                  int levels, double threshold, int sweeps, int coarse_sweeps, double line_threshold,
                                  const double* d_v, double* d_z, int* nlevels)
{
	return fvhip_amg_precondition_smoother_device(h, d_diag, d_lower, d_upper, levels, threshold, sweeps, coarse_sweeps,
	                                              line_threshold, d_v, d_z, nlevels, 0, 0);
}

int fvhip_amg_precondition_smoother_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                           int levels, double threshold, int sweeps, int coarse_sweeps, double line_threshold,
                                           const double* d_v, double* d_z, int* nlevels, int smoother, int block_rows)
{
	return guard([&] {
		need(h, "handle");
		needBlocks(h->L.ninface, d_diag, d_lower, d_upper);
		checkAmgCall(levels, sweeps, coarse_sweeps, d_v, d_z);
		const int rows = checkAmgSmoother(smoother, block_rows);
		System S = single(h);
		applyAmg(S, &d_diag, &d_lower, &d_upper, levels, threshold, sweeps, coarse_sweeps, line_threshold,
		         d_v ? &d_v : nullptr, &d_z, smoother, rows);
		if(nlevels) *nlevels = static_cast<int>(h->amg.size());
	});
}

int fvhip_group_amg_precondition_smoother_device(fvhip_group g, const double* const* d_diag, const double* const* d_lower,
                                                 const double* const* d_upper, int levels, double threshold, int sweeps,
                                                 int coarse_sweeps, double line_threshold, const double* const* d_v,
                                                 double* const* d_z, int* nlevels, int smoother, int block_rows)
{
	return guard([&] {
		need(g, "group");
		const size_t n = g->hs.size();
		needEach(d_diag, n, "diag");
		if(!d_lower || !d_upper) throw std::invalid_argument("null argument: lower / upper");
		for(size_t i = 0; i < n; i++) if(g->hs[i]->L.ninface > 0) { need(d_lower[i], "lower"); need(d_upper[i], "upper"); }
		checkAmgCall(levels, sweeps, coarse_sweeps, d_v, d_z);
		if(d_v) { needEach(d_v, n, "v"); needEach(d_z, n, "z"); }
		const int rows = checkAmgSmoother(smoother, block_rows);
		System S = ofGroup(g);
		applyAmg(S, d_diag, d_lower, d_upper, levels, threshold, sweeps, coarse_sweeps, line_threshold, d_v, d_z, smoother, rows);
		if(nlevels) for(size_t i = 0; i < n; i++) nlevels[i] = static_cast<int>(S.hs[i]->amg.size());
	});
}

int fvhip_amg_level(fvhip_handle h, int level, int* n, int* nnz, int* agg, int* rowptr, int* col, double* val)
{
	return guard([&] {
		const AmgLevel& L = amgLevelOf(h, level);
		HC(hipSetDevice(h->device));
		HC(hipStreamSynchronize(h->stream));
		if(n) *n = L.n;
		if(nnz) *nnz = L.nnz;
		if(agg) HC(hipMemcpy(agg, L.agg, sizeof(int)*static_cast<size_t>(L.nfine), hipMemcpyDeviceToHost));
		if(rowptr) HC(hipMemcpy(rowptr, L.rowptr, sizeof(int)*(static_cast<size_t>(L.n) + 1), hipMemcpyDeviceToHost));
		if(col) HC(hipMemcpy(col, L.col, sizeof(int)*static_cast<size_t>(L.nnz), hipMemcpyDeviceToHost));
		if(val) HC(hipMemcpy(val, L.val, 16*sizeof(double)*static_cast<size_t>(L.nnz), hipMemcpyDeviceToHost));
	});
}

int fvhip_amg_smooth_level_device(fvhip_handle h, int level, int smoother, int block_rows, int sweeps, int direction,
                                  int zero, const double* d_b, double* d_x)
{
	return guard([&] {
		AmgLevel& C = amgLevelOf(h, level);
		need(d_b, "b"); need(d_x, "x");
		if(smoother != 0 && smoother != 1) throw std::invalid_argument("smoother must be 0 or 1");
		if(sweeps < 1) throw std::invalid_argument("sweeps >= 1");
		if(direction < 0 || direction > 2) throw std::invalid_argument("direction must be 0 (forward), 1 (backward) or 2 (alternating)");
		HC(hipSetDevice(h->device));
		const int rows = smoother == 1 ? amgBlockRows(block_rows) : 0;
		smoothLevel(h, C, smoother, rows, d_b, d_x, sweeps, direction, zero != 0);
		HC(hipGetLastError());
		HC(hipStreamSynchronize(h->stream));
	});
}

int fvhip_amg_level_colours(fvhip_handle h, int level, int* ncolours, int* colour)
{
	return guard([&] {
		const AmgLevel& C = amgLevelOf(h, level);
		const int nc = static_cast<int>(C.cstart_colour.size()) - 1;
		if(ncolours) *ncolours = nc;
		if(colour)
			for(int q = 0; q < nc; q++)
				for(int k = C.cstart_colour[q]; k < C.cstart_colour[q+1]; k++) colour[C.h_cells[k]] = q;
	});
}

int fvhip_amg_level_blocks(fvhip_handle h, int level, int block_rows, int* nblocks, int* offsets)
{
	return guard([&] {
		AmgLevel& C = amgLevelOf(h, level);
		const int R = amgBlockRows(block_rows);
		HC(hipSetDevice(h->device));
		h->amgBlocks(C, R);
		const std::vector<int>& off = C.blocks[R].off;
		if(nblocks) *nblocks = (C.n + R - 1)/R;
		if(offsets) std::copy(off.begin(), off.end(), offsets);
	});
}

int fvhip_colouring(fvhip_handle h, int* ncolours, int* colour, long long* triples)
{
	return guard([&] {
		need(h, "handle");
		h->ensureColouring();
		if(ncolours) *ncolours = static_cast<int>(h->gs_colour_start.size()) - 1;
		if(colour) std::copy(h->gs_colour.begin(), h->gs_colour.end(), colour);
		if(triples) *triples = h->gs_triples;
	});
}

int fvhip_lines(fvhip_handle h, double line_threshold, int* nlines, int* start, int* cells, int* faces)
{
	return guard([&] {
		need(h, "handle");
		HC(hipSetDevice(h->device));
		h->ensureLines(line_threshold);
		if(nlines) *nlines = h->lines.nlines;
		if(start) std::copy(h->h_line_start.begin(), h->h_line_start.end(), start);
		if(cells) std::copy(h->h_line_cells.begin(), h->h_line_cells.end(), cells);
		if(faces) std::copy(h->h_line_faces.begin(), h->h_line_faces.end(), faces);
	});
}

}
