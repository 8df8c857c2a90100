/** \file implicit.cpp
 * \brief Device-resident pseudo-time solvers over one global system:
 *   SteadyForwardEulerSolver::solve (aodesolver.cpp:135-282) and SteadyBackwardEulerSolver::solve
 *   (aodesolver.cpp:363-638), plus the partitioned matrix-free operator.
 *
 * The reference hands each linear system to PETSc (KSPSolve, aodesolver.cpp:483; GMRES with a
 * block-Jacobi/ILU or SOR preconditioner from the .solverc files). Here it is solved on the device
 * by restarted GMRES: right-preconditioned (the residual it monitors is the true one), classical
 * Gram-Schmidt with selective (DGKS) re-orthogonalisation (one fused multi-dot reduction, i.e. one
 * small host round trip, per Arnoldi step in the common case, a second only when the projection
 * cancelled more than half of |w|^2; modified Gram-Schmidt would take j+1), preconditioned by
 * block-Jacobi sweeps on the assembled first-order Jacobian. PETSc's ILU/SOR are sequential
 * recurrences; a block-Jacobi sweep is one launch over all cells, and several sweeps approach the
 * block Gauss-Seidel effect. The matrix-free operator (alinalg.cpp:142-233) uses the assembled
 * blocks as preconditioner, as the reference's KSPSetOperators(A_mf, M) does (casesolvers.cpp:170).
 *
 * A system is either one handle (one GPU, or one rank of a partition with its RCCL communicator:
 * partial sums combined by ncclAllReduce) or all ranks of a partition driven from one process (a
 * group: halo rows by device copies, partial sums added on the host in handle order).
 */
#include "ctx.hpp"

#include <cmath>
#include <vector>

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
	if(!(thr >= 0.0) || !std::isfinite(thr)) throw std::invalid_argument("line_threshold must be finite and >= 0 (0: 4)");
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

void fvhip_ctx::ensureAmg(int levels, double thr) {
	if(levels < 2) throw std::invalid_argument("prec_amg: at least 2 levels");
	if(!(thr >= 0.0 && thr < 1.0)) throw std::invalid_argument("amg_threshold must be in [0, 1)");
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

namespace fvhip_detail {

struct System
{
	std::vector<fvhip_ctx*> hs;
	fvhip_ctx::GroupExchange exg;        ///< in-process halo transport of a group, else empty

	size_t size() const { return hs.size(); }
	bool halo() const { return hs[0]->halo(); }
	template <typename F> void each(F&& f) {
		for(size_t i = 0; i < hs.size(); i++) { HC(hipSetDevice(hs[i]->device)); f(i, hs[i]); }
	}
	void exchange(const fvhip_ctx::ArrayOf& arr, int width) {
		if(!halo()) return;
		if(exg) { exg(arr, width, 1); return; }
		each([&](size_t i, fvhip_ctx* h) { h->exchange_rccl(arr(i), width); });
	}
	/// global sums of k values every handle left in its iw.red, needed on the device only: one handle
	/// reduces over its ranks in place (ncclAllReduce, or nothing on one GPU) without a host round trip;
	/// a group sums on the host (allsum)
	void allsumDevice(int k) {
		if(hs.size() == 1) {
			fvhip_ctx* h = hs[0];
			if(h->comm) { HC(hipSetDevice(h->device)); NC(ncclAllReduce(h->iw.red, h->iw.red, k, ncclDouble, ncclSum, h->comm, h->stream)); }
			return;
		}
		allsum(k, true);
	}
	/// global sums of the k values every handle left in its iw.red: returned on the host and, if
	/// to_device, present in every handle's iw.red afterwards
	std::vector<double> allsum(int k, bool to_device) {
		each([&](size_t, fvhip_ctx* h) {
			if(h->comm) NC(ncclAllReduce(h->iw.red, h->iw.red, k, ncclDouble, ncclSum, h->comm, h->stream));
			HC(hipMemcpyAsync(h->iw.h_red, h->iw.red, k*sizeof(double), hipMemcpyDeviceToHost, h->stream));
		});
		std::vector<double> tot(k, 0.0);
		each([&](size_t, fvhip_ctx* h) {
			HC(hipStreamSynchronize(h->stream));
			for(int j = 0; j < k; j++) tot[j] += h->iw.h_red[j];
		});
		if(hs.size() > 1 && to_device)
			each([&](size_t, fvhip_ctx* h) {
				std::copy(tot.begin(), tot.end(), h->iw.h_red);
				HC(hipMemcpyAsync(h->iw.red, h->iw.h_red, k*sizeof(double), hipMemcpyHostToDevice, h->stream));
			});
		return tot;
	}
	void sync() { each([&](size_t, fvhip_ctx* h) { HC(hipStreamSynchronize(h->stream)); }); }
	/// one handle: the global sums of the k values in iw.red, copied to iw.h_red2 behind the reduction
	/// without waiting (read them after a later wait on the stream)
	void allsumQueue(int k) {
		fvhip_ctx* h = hs[0];
		HC(hipSetDevice(h->device));
		if(h->comm) NC(ncclAllReduce(h->iw.red, h->iw.red, k, ncclDouble, ncclSum, h->comm, h->stream));
		HC(hipMemcpyAsync(h->iw.h_red2, h->iw.red, k*sizeof(double), hipMemcpyDeviceToHost, h->stream));
	}
};

typedef fvhip_ctx::ArrayOf ArrayOf;

/// MatrixFreeSpatialJacobian::apply (alinalg.cpp:142-233) over a system: |x| is the global norm,
/// the perturbed state gets its ghost rows from the residual's own exchange
/// have_norm: |x|^2 is already in iw.red (the line solve that produced x summed it, LinOp::precondition)
static void matfreeApply(System& S, const ArrayOf& x, const ArrayOf& y, bool have_norm = false)
{
	S.each([&](size_t i, fvhip_ctx* h) {
		if(!h->mf_u || !h->mf_r || !h->mf_mdt) throw std::runtime_error("matrix-free operator: state not set");
		if(!have_norm) launch_mdot(4LL*h->L.ncell, 0, nullptr, 0, x(i), true, h->iw.part, h->iw.red, h->stream);
	});
	if(!have_norm) S.allsumDevice(1);          // |x|^2 stays on the device (launch_pertmag reads it there)
	if(S.size() == 1 && !S.exg && S.hs[0]->matfreeFusable() && S.hs[0]->matfreeNoAlias(S.hs[0]->mf_u, x(0), y(0))) {
		// one launch: the perturbed state and the combination inside the residual kernel (bitwise the same)
		fvhip_ctx* h = S.hs[0];
		launch_pertmag(h->iw.red, h->mf_eps, h->iw.pm, h->stream);
		h->matfree_fused(h->mf_u, x(0), h->iw.pm, h->mf_r, h->mf_mdt, y(0));
		HC(hipGetLastError());
		return;
	}
	std::vector<const double*> aux;
	std::vector<double*> yg, none(S.size(), nullptr);
	S.each([&](size_t i, fvhip_ctx* h) {
		launch_pertmag(h->iw.red, h->mf_eps, h->iw.pm, h->stream);
		launch_mf_perturb(4LL*h->L.ncell, h->mf_u, x(i), h->iw.pm, h->iw.aux, h->stream);
		aux.push_back(h->iw.aux);
		yg.push_back(h->iw.yg);
	});
	fvhip_ctx::residual_seq(S.hs, aux, yg, false, none, true, S.exg);
	S.each([&](size_t i, fvhip_ctx* h) {
		launch_mf_combine(h->L.ncell, h->mf_mdt, x(i), h->iw.yg, h->mf_r, h->iw.pm, y(i), h->stream);
		HC(hipGetLastError());
	});
}

/// amg_block_rows as given (0: the default) -> the block smoother's rows per block
static int amgBlockRows(int given)
{
	if(given == 0) return AMG_BLOCK_ROWS_DEFAULT;
	if(given < 64 || given > AMG_BLOCK_ROWS || given % 64 != 0)
		throw std::invalid_argument("amg_block_rows must be 0 (the default) or a multiple of 64 in [64, 2048]");
	return given;
}

/// `sweeps` sweeps of the block smoother (launch_amg_bjgs, blocks of R rows) on A_C x = b, the iterate in C.x
/// (taken as 0 if `zero`): each sweep reads C.x and writes C.x2, which then trade places, so the result is in
/// C.x again; from zero the first sweep reads no iterate and writes C.x itself. direction: 0 forward, 1 backward,
/// 2 alternating from forward
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

/// The linear operator and preconditioner of one implicit step
struct LinOp
{
	System& S;
	bool matfree = false;
	bool single = false;                      ///< preconditioner blocks in fp32 (iw.sdinv/slo/sup; line factors: LineSet::single)
	bool gs = false;                          ///< multicolour block Gauss-Seidel instead of Jacobi
	bool lines = false;                       ///< line-implicit (block-tridiagonal along lines)
	bool ilu = false;                         ///< block ILU(0): in multicolour order, or (ilu_order) sweep-based in a row order
	int ilu_order = 0;                        ///< 0: colour order; 1: internal order, 2: reverse Cuthill-McKee (sweep-based)
	int ilu_build = 0, ilu_apply = 0;         ///< sweep-based form: factor sweeps (>= 0) and solve sweeps (>= 1)
	double line_thr = 0.0;
	int sweeps = 1;
	int amg = 0;                              ///< aggregation multigrid levels (0: one-level preconditioner)
	int amg_sweeps = 2, amg_coarse = 6, amg_fine = 2;
	double amg_thr = 0.2;
	int amg_smoother = 0, amg_rows = AMG_BLOCK_ROWS_DEFAULT;   ///< coarse-level smoother (cycle) and its block rows
	std::vector<const double*> D, Lo, Up;     ///< per handle: diagonal / lower / upper blocks
	const ArrayOf aux = [this](size_t i) { return S.hs[i]->iw.aux; };   ///< each handle's scratch vectors
	const ArrayOf t = [this](size_t i) { return S.hs[i]->iw.t; };

	/// the preconditioner's blocks of handle i in the precision it applies them in (prec_single: the fp32
	/// copies setup() made): f(PrecBlocks); the launch_* overloads select on the pointer type
	template <typename T> struct PrecBlocks { const T *diag, *dinv, *lo, *up; };
	template <typename F> void withBlocks(size_t i, F&& f) {
		const fvhip_ctx::ImplicitWork& w = S.hs[i]->iw;
		if(single) f(PrecBlocks<float>{w.sdiag, w.sdinv, w.slo, w.sup});
		else f(PrecBlocks<double>{D[i], w.dinv, Lo[i], Up[i]});
	}

	/// y = A x with the assembled blocks; x has ghost rows, which are filled here
	void blocks(const ArrayOf& x, const ArrayOf& y) {
		S.exchange(x, 4);
		S.each([&](size_t i, fvhip_ctx* h) {
			h->timed("k_block_apply", [&]{ launch_block_apply(h->J, D[i], Lo[i], Up[i], x(i), y(i), h->stream); });
		});
	}
	/// set by a precondition call asked for the norm of its output (the Arnoldi step's z), consumed by the
	/// next apply: the matrix-free operator needs |z| and the line solve summed it while writing z
	bool znorm = false;
	void apply(const ArrayOf& x, const ArrayOf& y) {
		const bool have = znorm;
		znorm = false;
		if(matfree) matfreeApply(S, x, y, have);
		else blocks(x, y);
	}
	/// z = M^-1 v: `sweeps` block-Jacobi sweeps on A z = v from z = 0 (z has ghost rows). The iterates
	/// alternate between z and aux (both with ghost rows) so that the last one lands in z.
	void precondition(const ArrayOf& v, const ArrayOf& z, bool want_norm = false) {
		znorm = false;
		if(amg) { amgApply(v, z); return; }
		if(gs) { gaussSeidel(v, z); return; }
		if(lines) { lineSweeps(v, z, want_norm); return; }
		if(ilu) { iluSweeps(v, z); return; }
		auto buf = [&](int k) -> const ArrayOf& { return ((sweeps - 1 - k) % 2 == 0) ? z : aux; };
		S.each([&](size_t i, fvhip_ctx* h) {
			h->timed("k_bjac_apply", [&]{
				withBlocks(i, [&](auto B) { launch_bjac_apply(h->L.ncell, B.dinv, v(i), buf(0)(i), h->stream); });
			});
		});
		for(int k = 1; k < sweeps; k++) {
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
	void sweepColour(size_t i, int col, const double* v, double* z) {
		fvhip_ctx* h = S.hs[i];
		const int b = h->gs_colour_start[col], n = h->gs_colour_start[col+1] - b;
		withBlocks(i, [&](auto B) { launch_bgs_colour(h->J, B.dinv, B.lo, B.up, v, z, h->d_gs_cells + b, n, h->stream); });
	}
	/// z = M^-1 v by `sweeps` multicolour block Gauss-Seidel sweeps from z = 0, colours in forward
	/// then backward order on alternate sweeps (symmetric Gauss-Seidel pairs). Across ranks the
	/// sweep is block-Jacobi: ghost rows are exchanged once per sweep -- the reference's PETSc
	/// setting -pc_type bjacobi -sub_pc_type sor, with a colour order instead of a row order.
	void gaussSeidel(const ArrayOf& v, const ArrayOf& z) {
		S.each([&](size_t i, fvhip_ctx* h) {
			exact::launch_fill(z(i), 0.0, 4LL*(h->L.ncell + h->L.nghost), h->stream);
		});
		for(int k = 0; k < sweeps; k++) {
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
	void iluApply(const ArrayOf& v, const ArrayOf& z) {
		if(ilu_order) { iluSweepApply(v, z); return; }
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
	void iluSweepApply(const ArrayOf& v, const ArrayOf& z) {
		const int a = ilu_apply;
		S.each([&](size_t i, fvhip_ctx* h) {
			const int* rank = h->ensureIluOrder(ilu_order).d_rank;
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
	void iluSweeps(const ArrayOf& v, const ArrayOf& z) {
		iluApply(v, z);
		for(int k = 1; k < sweeps; k++) {
			blocks(z, t);
			S.each([&](size_t i, fvhip_ctx* h) { launch_axpby(4LL*h->L.ncell, 1.0, v(i), -1.0, t(i), h->stream); });
			iluApply(t, aux);
			S.each([&](size_t i, fvhip_ctx* h) { launch_add_rows(h->L.ncell, aux(i), z(i), h->stream); });
		}
	}
	/// z = M^-1 v with M the block-tridiagonal line part of A (factorised in setup), then `sweeps` - 1
	/// corrections z += M^-1 (v - A z) (A with the ghost coupling: block-Jacobi across ranks)
	void lineSweeps(const ArrayOf& v, const ArrayOf& z, bool want_norm = false) {
		// one sweep on one domain for the matrix-free operator: the line solve also returns |z|^2
		const bool norm = want_norm && matfree && sweeps == 1 && S.size() == 1 && !S.exg && !S.halo();
		S.each([&](size_t i, fvhip_ctx* h) {
			h->timed("k_line_solve", [&]{ launch_line_solve(h->lines, v(i), z(i), h->stream, norm ? h->iw.red : nullptr); });
		});
		znorm = norm;
		for(int k = 1; k < sweeps; k++) {
			blocks(z, t);
			S.each([&](size_t i, fvhip_ctx* h) {
				launch_axpby(4LL*h->L.ncell, 1.0, v(i), -1.0, t(i), h->stream);
				h->timed("k_line_solve", [&]{ launch_line_solve(h->lines, t(i), aux(i), h->stream); });
				launch_add_rows(h->L.ncell, aux(i), z(i), h->stream);
			});
		}
	}
	/// z = the finest smoother applied to v (line solve, else D^-1 v)
	void smooth0(fvhip_ctx* h, size_t i, const double* v, double* z) {
		if(lines) h->timed("k_line_solve", [&]{ launch_line_solve(h->lines, v, z, h->stream); });
		else withBlocks(i, [&](auto B) { launch_bjac_apply(h->L.ncell, B.dinv, v, z, h->stream); });
	}
	/// t = v - A z (A with the ghost coupling)
	void residual0(const ArrayOf& v, const ArrayOf& z, const ArrayOf& t) {
		S.exchange(z, 4);
		S.each([&](size_t i, fvhip_ctx* h) {
			h->timed("k_block_residual", [&]{
				withBlocks(i, [&](auto B) { launch_block_residual(h->J, B.diag, B.lo, B.up, z(i), v(i), t(i), h->stream); });
			});
		});
	}
	/// coarse level l of handle h's hierarchy: V-cycle on A_l x_l = b_l from x_l = 0 (colour Gauss-Seidel
	/// forward before the coarse correction, backward after it; the coarsest level amg_coarse sweeps,
	/// alternating). amg_smoother 0: Gauss-Seidel over the whole level; 1: inside row blocks of amg_rows rows,
	/// block-Jacobi between them (mgopts.solverc:31-32), same sweep counts and directions
	void cycle(fvhip_ctx* h, size_t l) {
		AmgLevel& C = h->amg[l];
		if(amg_smoother == 1) {          // block-Jacobi / Gauss-Seidel: one launch per sweep on a level of any size
			if(l + 1 == h->amg.size()) { amgBlockSweeps(h, C, amg_rows, C.b, amg_coarse, 2, true); return; }
			amgBlockSweeps(h, C, amg_rows, C.b, amg_sweeps, 0, true);
			launch_amg_residual(C, C.x, C.b, C.r, h->stream);
			AmgLevel& F = h->amg[l+1];
			launch_amg_restrict(F, C.r, F.b, h->stream);
			cycle(h, l + 1);
			launch_amg_prolong(F, F.x, C.x, h->stream);
			amgBlockSweeps(h, C, amg_rows, C.b, amg_sweeps, 1, false);
			return;
		}
		const bool small = C.n <= AMG_BLOCK_ROWS;        // one workgroup sweeps the level (no launch per colour)
		if(!small) exact::launch_fill(C.x, 0.0, 4LL*C.n, h->stream);
		const int nc = static_cast<int>(C.cstart_colour.size()) - 1;
		auto sweep = [&](bool fwd) {
			for(int q = 0; q < nc; q++) launch_amg_gs_colour(C, fwd ? q : nc - 1 - q, C.b, C.x, h->stream);
		};
		if(l + 1 == h->amg.size()) {
			if(small) launch_amg_gs_block(C, C.b, C.x, amg_coarse, true, true, true, h->stream);
			else for(int k = 0; k < amg_coarse; k++) sweep(k % 2 == 0);
			return;
		}
		if(small) launch_amg_gs_block(C, C.b, C.x, amg_sweeps, true, false, true, h->stream);
		else for(int k = 0; k < amg_sweeps; k++) sweep(true);
		launch_amg_residual(C, C.x, C.b, C.r, h->stream);
		AmgLevel& F = h->amg[l+1];
		launch_amg_restrict(F, C.r, F.b, h->stream);
		cycle(h, l + 1);
		launch_amg_prolong(F, F.x, C.x, h->stream);
		if(small) launch_amg_gs_block(C, C.b, C.x, amg_sweeps, false, false, false, h->stream);
		else for(int k = 0; k < amg_sweeps; k++) sweep(false);
	}
	/// z = M^-1 v, M one V-cycle of the aggregation multigrid (block-Jacobi across ranks: each handle's hierarchy
	/// covers its owned cells; the finest residuals include the ghost coupling)
	void amgApply(const ArrayOf& v, const ArrayOf& z) {
		S.each([&](size_t i, fvhip_ctx* h) { smooth0(h, i, v(i), z(i)); });
		auto correct = [&]() {             // z += M0^-1 (v - A z)
			residual0(v, z, t);
			S.each([&](size_t i, fvhip_ctx* h) { smooth0(h, i, t(i), aux(i)); launch_add_rows(h->L.ncell, aux(i), z(i), h->stream); });
		};
		for(int k = 1; k < amg_fine; k++) correct();
		residual0(v, z, t);
		S.each([&](size_t i, fvhip_ctx* h) {
			h->timed("k_amg_cycle", [&]{
				launch_amg_restrict(h->amg[0], t(i), h->amg[0].b, h->stream);
				cycle(h, 0);
				launch_amg_prolong(h->amg[0], h->amg[0].x, z(i), h->stream);
			});
		});
		for(int k = 0; k < amg_fine; k++) correct();
	}
	/// the preconditioner of the current blocks: the line factorisation or the (ILU) diagonal inverses -- with
	/// the multigrid, its finest smoother -- their fp32 copies, and the multigrid's coarse operators.
	/// (The entry points refuse prec_lines with prec_gs / prec_ilu, and the multigrid with either.)
	void setup() {
		S.each([&](size_t i, fvhip_ctx* h) {
			const fvhip_ctx::ImplicitWork& w = h->iw;
			if(lines) {
				h->ensureLines(line_thr);
				h->lines.single = single;
				h->timed("k_line_factor", [&]{ launch_line_factor(h->lines, D[i], Lo[i], Up[i], h->stream); });
			} else if(ilu && ilu_order) h->iluSweepFactor(ilu_order, ilu_build, D[i], Lo[i], Up[i], w.dinv);
			else if(ilu) h->iluFactor(D[i], Lo[i], Up[i], w.dinv);
			else h->timed("k_bjac_invert", [&]{ launch_bjac_invert(h->L.ncell, D[i], w.dinv, h->stream); });
			if(gs) h->ensureColouring();
			if(single && (amg || !lines)) {      // (the line factors are stored in fp32 by the factorisation itself)
				h->ensureSinglePrecond();
				const long long nd = 16LL*h->L.ncell, nf = 16LL*std::max(h->L.ninface, 0);
				auto convert = [&](long long n, const double* a, float* b) { launch_to_single(n, a, b, h->stream); };
				h->timed("k_to_single", [&]{
					if(amg) convert(nd, D[i], w.sdiag);      // the finest operator, for the smoother's residuals
					else convert(nd, w.dinv, w.sdinv);
					if(amg || sweeps > 1 || gs || ilu) { convert(nf, Lo[i], w.slo); convert(nf, Up[i], w.sup); }
					if(amg && !lines) convert(nd, w.dinv, w.sdinv);
				});
			}
			if(amg) {
				h->ensureAmg(amg, amg_thr);
				h->amgSetup(D[i], Lo[i], Up[i]);
			}
		});
	}
};

struct GmresOut { int iters; double rnorm0, rnorm; };

/// Restarted GMRES(m) for A x = b, x0 = 0; stops when |b - A x| <= rtol |b| or after maxit
/// Arnoldi steps in total (KSPSolve with -ksp_rtol, -ksp_max_it, -ksp_gmres_restart)
static GmresOut gmres(System& S, LinOp& A, const ArrayOf& b, const ArrayOf& x, double rtol, int maxit, int m,
                      int refine = 0)
{
	if(refine < 0 || refine > 2) throw std::invalid_argument("cgs_refine must be 0 (never), 1 (ifneeded) or 2 (always)");
	auto n4 = [&](size_t i) { return 4LL*S.hs[i]->L.ncell; };
	auto V = [&](size_t i, int j) { return S.hs[i]->iw.V + static_cast<size_t>(j)*static_cast<size_t>(n4(i)); };
	const ArrayOf z = [&](size_t i) { return S.hs[i]->iw.z; };
	const ArrayOf w = [&](size_t i) { return S.hs[i]->iw.w; };
	const ArrayOf sv = [&](size_t i) { return S.hs[i]->iw.s; };
	auto norm = [&](const ArrayOf& v) {
		S.each([&](size_t i, fvhip_ctx* h) { launch_mdot(n4(i), 0, nullptr, 0, v(i), true, h->iw.part, h->iw.red, h->stream); });
		return std::sqrt(S.allsum(1, false)[0]);
	};
	S.each([&](size_t i, fvhip_ctx* h) { exact::launch_fill(x(i), 0.0, n4(i), h->stream); });
	const double beta0 = norm(b);
	GmresOut out{0, beta0, beta0};
	if(!(beta0 > 0.0) || maxit <= 0) return out;

	std::vector<double> H(static_cast<size_t>(m+1)*m, 0.0), cs(m), sn(m), g(m+1), y(m);
	auto Hij = [&](int i, int j) -> double& { return H[static_cast<size_t>(j)*(m+1) + i]; };
	double beta = beta0;
	bool first = true;
	while(true) {
		if(first) S.each([&](size_t i, fvhip_ctx* h) { launch_axpby(n4(i), 1.0/beta, b(i), 0.0, V(i,0), h->stream); });
		else {
			// restart: r = b - A x (x into the ghosted operand buffer first)
			S.each([&](size_t i, fvhip_ctx* h) {
				HC(hipMemcpyAsync(z(i), x(i), n4(i)*sizeof(double), hipMemcpyDeviceToDevice, h->stream));
			});
			A.apply(z, w);
			S.each([&](size_t i, fvhip_ctx* h) { launch_axpby(n4(i), 1.0, b(i), -1.0, w(i), h->stream); });
			beta = norm(w);
			out.rnorm = beta;
			if(beta <= rtol*beta0) break;
			S.each([&](size_t i, fvhip_ctx* h) { launch_axpby(n4(i), 1.0/beta, w(i), 0.0, V(i,0), h->stream); });
		}
		std::fill(g.begin(), g.end(), 0.0);
		g[0] = beta;
		int j = 0;
		bool done = false;
		while(j < m && out.iters < maxit) {
			A.precondition([&](size_t i) { return V(i,j); }, z, true);
			A.apply(z, w);
			// classical Gram-Schmidt (PETSc's KSPGMRESClassicalGramSchmidtOrthogonalization). refine 0
			// (PETSc's default, KSP_GMRES_CGS_REFINE_NEVER): one projection h = V^T w, w -= V h, and the new
			// norm computed from the projected w in the same pass (k_maxpy_norm) -- two passes over the
			// basis per step. refine 1 (ifneeded): the projection pass also returns |w|^2, so |w - V h|^2
			// follows by Pythagoras and a second projection runs only when the first removed more than half
			// of |w|^2 (DGKS); refine 2 (always): two projections every step.
			double hn2 = 0.0;
			if(refine == 0 && S.size() == 1) {
				// one handle: the projection's coefficients stay on the device for k_maxpy_norm and reach
				// the host with its norm -- one wait per Arnoldi step
				fvhip_ctx* h = S.hs[0];
				launch_mdot(n4(0), j+1, V(0,0), n4(0), w(0), false, h->iw.part, h->iw.red, h->stream);
				S.allsumQueue(j+1);
				launch_maxpy_norm(n4(0), j+1, V(0,0), n4(0), h->iw.red, w(0), h->iw.part, h->iw.red, h->stream);
				hn2 = S.allsum(1, false)[0];
				for(int k = 0; k <= j; k++) Hij(k,j) = h->iw.h_red2[k];
			} else if(refine != 1) {
				S.each([&](size_t i, fvhip_ctx* h) {
					launch_mdot(n4(i), j+1, V(i,0), n4(i), w(i), false, h->iw.part, h->iw.red, h->stream);
				});
				const std::vector<double> h1 = S.allsum(j+1, true);
				for(int k = 0; k <= j; k++) Hij(k,j) = h1[k];
				if(refine == 2) {
					S.each([&](size_t i, fvhip_ctx* h) { launch_maxpy(n4(i), j+1, V(i,0), n4(i), h->iw.red, w(i), h->stream); });
					S.each([&](size_t i, fvhip_ctx* h) {
						launch_mdot(n4(i), j+1, V(i,0), n4(i), w(i), false, h->iw.part, h->iw.red, h->stream);
					});
					const std::vector<double> h2 = S.allsum(j+1, true);
					for(int k = 0; k <= j; k++) Hij(k,j) += h2[k];
				}
				S.each([&](size_t i, fvhip_ctx* h) {
					launch_maxpy_norm(n4(i), j+1, V(i,0), n4(i), h->iw.red, w(i), h->iw.part, h->iw.red, h->stream);
				});
				hn2 = S.allsum(1, false)[0];
			} else {
				S.each([&](size_t i, fvhip_ctx* h) {
					launch_mdot(n4(i), j+1, V(i,0), n4(i), w(i), true, h->iw.part, h->iw.red, h->stream);
				});
				const std::vector<double> h1 = S.allsum(j+2, true);
				S.each([&](size_t i, fvhip_ctx* h) { launch_maxpy(n4(i), j+1, V(i,0), n4(i), h->iw.red, w(i), h->stream); });
				double corr = 0.0;
				for(int k = 0; k <= j; k++) { Hij(k,j) = h1[k]; corr += h1[k]*h1[k]; }
				hn2 = h1[j+1] - corr;
				if(!(hn2 > 0.5*h1[j+1])) {
					S.each([&](size_t i, fvhip_ctx* h) {
						launch_mdot(n4(i), j+1, V(i,0), n4(i), w(i), true, h->iw.part, h->iw.red, h->stream);
					});
					const std::vector<double> h2 = S.allsum(j+2, true);
					S.each([&](size_t i, fvhip_ctx* h) { launch_maxpy(n4(i), j+1, V(i,0), n4(i), h->iw.red, w(i), h->stream); });
					corr = 0.0;
					for(int k = 0; k <= j; k++) { Hij(k,j) += h2[k]; corr += h2[k]*h2[k]; }
					hn2 = h2[j+1] - corr;
					if(!(hn2 > 1e-4*h2[j+1])) { const double t = norm(w); hn2 = t*t; }   // cancellation: measure
				}
			}
			const double hn = std::sqrt(hn2);
			Hij(j+1,j) = hn;
			if(hn > 0.0) S.each([&](size_t i, fvhip_ctx* h) { launch_axpby(n4(i), 1.0/hn, w(i), 0.0, V(i,j+1), h->stream); });
			// Givens rotations of the Hessenberg column
			for(int k = 0; k < j; k++) {
				const double t = cs[k]*Hij(k,j) + sn[k]*Hij(k+1,j);
				Hij(k+1,j) = -sn[k]*Hij(k,j) + cs[k]*Hij(k+1,j);
				Hij(k,j) = t;
			}
			const double d = std::hypot(Hij(j,j), Hij(j+1,j));
			cs[j] = d > 0.0 ? Hij(j,j)/d : 1.0;
			sn[j] = d > 0.0 ? Hij(j+1,j)/d : 0.0;
			Hij(j,j) = d; Hij(j+1,j) = 0.0;
			g[j+1] = -sn[j]*g[j];
			g[j] = cs[j]*g[j];
			j++;
			out.iters++;
			out.rnorm = std::fabs(g[j]);
			if(!std::isfinite(out.rnorm)) throw std::runtime_error("GMRES: non-finite residual");
			if(out.rnorm <= rtol*beta0 || hn == 0.0) { done = true; break; }
		}
		// x += M^-1 V y with H y = g (upper triangular after the rotations)
		for(int k = j-1; k >= 0; k--) {
			double s = g[k];
			for(int l = k+1; l < j; l++) s -= Hij(k,l)*y[l];
			y[k] = s/Hij(k,k);
		}
		S.each([&](size_t i, fvhip_ctx* h) {
			std::copy(y.begin(), y.begin() + j, h->iw.h_coef);
			HC(hipMemcpyAsync(h->iw.coef, h->iw.h_coef, j*sizeof(double), hipMemcpyHostToDevice, h->stream));
			launch_lincomb(n4(i), j, V(i,0), n4(i), h->iw.coef, sv(i), h->stream);
		});
		A.precondition(sv, z);
		S.each([&](size_t i, fvhip_ctx* h) { launch_axpby(n4(i), 1.0, z(i), 1.0, x(i), h->stream); });
		S.sync();            // h_coef is rewritten by the next cycle
		if(done || out.iters >= maxit) break;
		first = false;
	}
	return out;
}

/// SteadySolver::expResidualRamp (aodesolver.cpp:110-120)
static double expResidualRamp(double cflmin, double cflmax, double prevcfl, double resratio,
                              double paramup, double paramdown)
{
	const double newcfl = resratio > 1.0 ? prevcfl * std::pow(resratio, paramup)
		: prevcfl * std::pow(resratio, paramdown);
	if(newcfl < cflmin) return cflmin;
	else if(newcfl > cflmax) return cflmax;
	else return newcfl;
}

/// the sweep-based ILU's options (fvhip_implicit_config::ilu_order / ilu_build_sweeps / ilu_apply_sweeps, and the
/// stand-alone call's arguments); all zero: the colour-order ILU or none
static void checkIluSweeps(int order, int build, int apply, bool prec_ilu)
{
	if(order < 0 || order > 2) throw std::invalid_argument("ilu_order must be 0 (colour order), 1 (internal order) or 2 (reverse Cuthill-McKee)");
	if(build < 0) throw std::invalid_argument("ilu_build_sweeps must be >= 0");
	if(apply < 0) throw std::invalid_argument("ilu_apply_sweeps must be >= 0");
	if(order == 0 && build != 0) throw std::invalid_argument("ilu_build_sweeps needs ilu_order 1 or 2");
	if(order == 0 && apply != 0) throw std::invalid_argument("ilu_apply_sweeps needs ilu_order 1 or 2");
	if(order != 0 && !prec_ilu) throw std::invalid_argument("ilu_order needs prec_ilu");
	if(order != 0 && apply < 1) throw std::invalid_argument("ilu_apply_sweeps must be >= 1 with ilu_order 1 or 2");
}

static void checkImplicit(const fvhip_implicit_config& c)
{
	checkIluSweeps(c.ilu_order, c.ilu_build_sweeps, c.ilu_apply_sweeps, c.prec_ilu != 0);
	if(c.restart < 1 || c.restart > KRY_MAXK) throw std::invalid_argument("restart must be in [1, 128]");
	if(c.cgs_refine < 0 || c.cgs_refine > 2) throw std::invalid_argument("cgs_refine must be 0 (never), 1 (ifneeded) or 2 (always)");
	if(c.prec_sweeps < 1) throw std::invalid_argument("prec_sweeps must be >= 1");
	if(c.prec_amg != 0 && c.prec_amg < 2) throw std::invalid_argument("prec_amg must be 0 (off) or >= 2 levels");
	if(c.amg_sweeps < 0 || c.amg_coarse_sweeps < 0 || c.amg_fine_sweeps < 0 || !(c.amg_threshold >= 0.0 && c.amg_threshold < 1.0))
		throw std::invalid_argument("amg_sweeps / amg_coarse_sweeps must be >= 0 and amg_threshold in [0, 1)");
	if(c.amg_smoother != 0 && c.amg_smoother != 1)
		throw std::invalid_argument("amg_smoother must be 0 (Gauss-Seidel over the level) or 1 (block-Jacobi / Gauss-Seidel)");
	if(c.amg_smoother == 1 && c.prec_amg == 0) throw std::invalid_argument("amg_smoother = 1 needs prec_amg");
	(void)amgBlockRows(c.amg_block_rows);
	if(!(c.min_relax > 0.0)) throw std::domain_error("Minimum relaxation factor is invalid!");  // nonlinearrelaxation.cpp:20-21
	if(c.matrix_free && !(c.mf_eps > 0.0)) throw std::invalid_argument("matrix-free difference step must be positive");
	if(!(c.line_threshold >= 0.0) || !std::isfinite(c.line_threshold))
		throw std::invalid_argument("line_threshold must be finite and >= 0 (0: the default 4)");
}

/// SteadyBackwardEulerSolver::solve (aodesolver.cpp:363-638) on device states us (internal order,
/// ghost rows included on partitioned handles)
static void backwardEuler(System& S, const std::vector<double*>& us, const fvhip_implicit_config& c,
                          fvhip_solve_stats* st, double* hist)
{
	checkImplicit(c);
	S.each([&](size_t, fvhip_ctx* h) { h->ensureImplicit(c.restart); h->mf_eps = c.mf_eps; });
	LinOp A{S};
	A.matfree = c.matrix_free != 0;
	A.sweeps = c.prec_sweeps;
	A.single = c.prec_single != 0;
	A.gs = c.prec_gs != 0;
	A.lines = c.prec_lines != 0;
	A.line_thr = c.line_threshold;
	A.ilu = c.prec_ilu != 0;
	A.ilu_order = c.ilu_order; A.ilu_build = c.ilu_build_sweeps; A.ilu_apply = c.ilu_apply_sweeps;
	if(A.lines && A.gs) throw std::invalid_argument("prec_lines does not combine with prec_gs");
	if(A.ilu && (A.gs || A.lines)) throw std::invalid_argument("prec_ilu does not combine with prec_gs / prec_lines");
	A.amg = c.prec_amg;
	A.amg_sweeps = c.amg_sweeps > 0 ? c.amg_sweeps : 2;
	A.amg_coarse = c.amg_coarse_sweeps > 0 ? c.amg_coarse_sweeps : 6;
	A.amg_fine = c.amg_fine_sweeps > 0 ? c.amg_fine_sweeps : A.amg_sweeps;
	A.amg_thr = c.amg_threshold > 0.0 ? c.amg_threshold : 0.2;
	A.amg_smoother = c.amg_smoother;
	A.amg_rows = amgBlockRows(c.amg_block_rows);
	if(A.amg && (A.gs || A.ilu || A.sweeps != 1))
		throw std::invalid_argument("prec_amg combines with prec_lines and prec_single only (prec_gs / prec_ilu / prec_sweeps > 1 are one-level options)");
	for(fvhip_ctx* h : S.hs) { A.D.push_back(h->iw.jd); A.Lo.push_back(h->iw.jlo); A.Up.push_back(h->iw.jup); }
	std::vector<const double*> cu(us.begin(), us.end());
	std::vector<double*> rs, dts;
	for(fvhip_ctx* h : S.hs) { rs.push_back(h->d_r); dts.push_back(h->d_dtm); }
	const ArrayOf bs = [&](size_t i) { return S.hs[i]->d_r; };
	const ArrayOf xs = [&](size_t i) { return S.hs[i]->iw.du; };

	double curCFL = 0, resi = 1.0, resiold = 1.0, initres = 1.0, linworst = 0.0;
	int step = 0, lin = 0, linbad = 0;
	const bool resume = c.resume_res0 > 0.0;
	if(resume) {                     // a checkpointed solve: its residuals and CFL, the ramp continues from them
		if(!(c.resume_res > 0.0 && c.resume_res_prev > 0.0 && c.resume_cfl > 0.0))
			throw std::invalid_argument("resume: the last residual, the one before and the last CFL must be positive");
		initres = c.resume_res0; resi = c.resume_res; resiold = c.resume_res_prev; curCFL = c.resume_cfl;
	}
	while(resi/initres > c.tol && step < c.maxiter) {
		// r = 0 + (-r(u)) with local time steps (:421-452); fills the ghost rows of u
		fvhip_ctx::residual_seq(S.hs, cu, rs, true, dts, true, S.exg);
		curCFL = expResidualRamp(c.cflinit, c.cflfin, curCFL, resiold/resi, 0.25, 0.3);           // :462
		// Jacobian (:456-457) with the pseudo-time term (:467) added in its diagonal pass
		S.each([&](size_t i, fvhip_ctx* h) { h->assemble(us[i], h->iw.jd, h->iw.jlo, h->iw.jup, curCFL, h->d_dtm); });
		A.setup();
		if(A.matfree)                                                                               // :386-394
			S.each([&](size_t i, fvhip_ctx* h) { h->mf_u = us[i]; h->mf_r = h->d_r; h->mf_mdt = h->d_dtm; });
		const GmresOut g = gmres(S, A, bs, xs, c.lin_rtol, c.lin_maxit, c.restart, c.cgs_refine);    // :483
		lin += g.iters;
		if(g.rnorm0 > 0.0) {
			linworst = std::max(linworst, g.rnorm/g.rnorm0);
			if(g.rnorm > c.lin_rtol*g.rnorm0) linbad++;
		}
		S.each([&](size_t i, fvhip_ctx* h) {                                                        // :494-512
			launch_relaxed_update(h->L.ncell, h->P.gas, c.min_relax, h->iw.du, us[i], h->stream);
			launch_energy_sumsq(h->L.ncell, h->d_r, h->M.area, h->iw.part, h->iw.red, h->stream);   // :516-526
			HC(hipGetLastError());
		});
		resiold = resi;
		resi = std::sqrt(S.allsum(1, false)[0]);                                                    // :528-530
		if(!std::isfinite(resi))
			throw std::runtime_error("Steady backward Euler diverged - residual is Nan or inf!");  // :533-534
		if(step == 0 && !resume) initres = resi;
		step++;
		if(hist) hist[step-1] = resi;
	}
	if(A.matfree) S.each([&](size_t, fvhip_ctx* h) { h->mf_u = h->mf_r = h->mf_mdt = nullptr; });
	st->steps = step;
	st->lin_iters = lin;
	st->resratio = resi/initres;
	st->converged = (step < c.maxiter && resi/initres <= c.tol) ? 1 : 0;                            // :618-632
	st->cfl = curCFL;
	st->lin_unconverged = linbad;
	st->lin_worst = linworst;
}

/// SteadyForwardEulerSolver::solve (aodesolver.cpp:135-282): u += cflinit dtm/area r (the ramped
/// CFL is only reported by the reference, :194, :208)
static void forwardEuler(System& S, const std::vector<double*>& us, double cfl, double tol, int maxiter,
                         int* steps, double* resratio, double* hist)
{
	S.each([&](size_t, fvhip_ctx* h) { h->ensureReductions(); });
	std::vector<const double*> cu(us.begin(), us.end());
	std::vector<double*> rs, dts;
	for(fvhip_ctx* h : S.hs) { rs.push_back(h->d_r); dts.push_back(h->d_dtm); }
	double resi = 1.0, initres = 1.0;
	int step = 0;
	while(resi/initres > tol && step < maxiter) {
		fvhip_ctx::residual_seq(S.hs, cu, rs, true, dts, true, S.exg);                          // :180-189
		S.each([&](size_t i, fvhip_ctx* h) {
			launch_fe_update(h->L.ncell, h->d_r, h->d_dtm, h->M.area, cfl, us[i], h->stream);   // :204-209
			launch_energy_sumsq(h->L.ncell, h->d_r, h->M.area, h->iw.part, h->iw.red, h->stream);
			HC(hipGetLastError());
		});
		resi = std::sqrt(S.allsum(1, false)[0]);                                                  // :214-230
		if(step == 0) initres = resi;
		if(hist) hist[step] = resi;
		step++;
		if(!std::isfinite(resi))
			throw std::runtime_error("Steady forward Euler diverged - residual is Nan or inf!");  // :250-251
	}
	if(steps) *steps = step;
	if(resratio) *resratio = resi/initres;
}

/// TVDRKSolver::solve (aodesolver.cpp:669-758) on the device, restated as written: ustage = u once
/// before the time loop (:701-704); per step, every stage's residual is computed at u -- the step's
/// start state, since the reference passes uvec, not the stage state, to compute_residual (:719) --
/// dtmin = min over cells of the first stage's local time steps (:722-728; across ranks the global
/// minimum, so a partitioned run takes the 1-GPU steps, where the reference's ranks would each take
/// their own), ustage = c0 u + c1 ustage - c2 dtmin cfl / area r (:735-744), then u = ustage and
/// time += dtmin cfl (:747-757), while time <= finaltime - 1e-12 (A_SMALL_NUMBER). The stages' residuals
/// are the same bits (same input, deterministic kernels), so one residual per step is computed and
/// reused. maxsteps caps the loop (the reference has no cap).
static void tvdrk(System& S, const std::vector<double*>& us, int order, double cfl, double finaltime, int maxsteps,
                  int* steps, double* time_out)
{
	static const double coef[3][3][3] = {                                       // initialize_TVDRK_Coeffs :45-67
		{{1.0, 0.0, 1.0}, {0, 0, 0}, {0, 0, 0}},
		{{1.0, 0.0, 1.0}, {0.5, 0.5, 0.5}, {0, 0, 0}},
		{{1.0, 0.0, 1.0}, {0.75, 0.25, 0.25}, {0.3333333333333333, 0.6666666666666667, 0.6666666666666667}}};
	if(order < 1 || order > 3) throw std::invalid_argument("TVD RK: temporal order must be 1, 2 or 3");
	if(maxsteps < 1) throw std::invalid_argument("TVD RK: maxsteps must be >= 1");
	const double (*tc)[3] = coef[order-1];
	S.each([&](size_t i, fvhip_ctx* h) {
		h->ensureReductions();
		if(!h->d_ustage) h->d_ustage = dalloc(4*static_cast<size_t>(std::max(h->L.ncell, 1)), h->owned);
		HC(hipMemcpyAsync(h->d_ustage, us[i], sizeof(double)*4*static_cast<size_t>(h->L.ncell), hipMemcpyDeviceToDevice,
		                  h->stream));
	});
	std::vector<const double*> cu(us.begin(), us.end());
	std::vector<double*> rs, dts;
	for(fvhip_ctx* h : S.hs) { rs.push_back(h->d_r); dts.push_back(h->d_dtm); }
	int step = 0;
	double time = 0;
	while(time <= finaltime - 1e-12 && step < maxsteps) {
		fvhip_ctx::residual_seq(S.hs, cu, rs, true, dts, true, S.exg);              // :712-719 (zeroed, -r(u))
		S.each([&](size_t, fvhip_ctx* h) {
			launch_min(h->L.ncell, h->d_dtm, h->iw.part, h->iw.red, h->stream);
			if(h->comm) NC(ncclAllReduce(h->iw.red, h->iw.red, 1, ncclDouble, ncclMin, h->comm, h->stream));
			HC(hipMemcpyAsync(h->iw.h_red, h->iw.red, sizeof(double), hipMemcpyDeviceToHost, h->stream));
		});
		double dtmin = INFINITY;
		S.each([&](size_t, fvhip_ctx* h) { HC(hipStreamSynchronize(h->stream)); dtmin = std::min(dtmin, h->iw.h_red[0]); });
		if(!std::isfinite(dtmin)) throw std::runtime_error("TVDRK solver diverged - dtmin is Nan or inf!");   // :730-731
		for(int s = 0; s < order; s++) {
			const double sc = tc[s][2]*dtmin*cfl;
			S.each([&](size_t i, fvhip_ctx* h) {
				launch_tvdrk_stage(h->L.ncell, tc[s][0], tc[s][1], sc, h->M.area, h->d_r, us[i], h->d_ustage, h->stream);
			});
		}
		S.each([&](size_t i, fvhip_ctx* h) {
			HC(hipMemcpyAsync(us[i], h->d_ustage, sizeof(double)*4*static_cast<size_t>(h->L.ncell), hipMemcpyDeviceToDevice,
			                  h->stream));
			HC(hipGetLastError());
		});
		step++;
		time += dtmin*cfl;
	}
	if(steps) *steps = step;
	if(time_out) *time_out = time;
}

static System single(fvhip_ctx* h)
{
	if(h->in_group) throw std::runtime_error("handle belongs to a group: use the fvhip_group_* entry point");
	if(h->halo() && !h->comm) throw std::runtime_error("partitioned handle: call fvhip_comm_init (or use a group) first");
	return System{{h}, {}};
}

static System ofGroup(fvhip_group_s* g) { return System{g->hs, groupExchange(g)}; }

void sysMatfree(const std::vector<fvhip_ctx*>& hs, const fvhip_ctx::GroupExchange& exg,
                const std::vector<const double*>& x, const std::vector<double*>& y)
{
	System S{hs, exg};
	S.each([&](size_t, fvhip_ctx* h) { h->ensureVectors(); });
	const ArrayOf xo = [&](size_t i) { return const_cast<double*>(x[i]); };
	const ArrayOf yo = [&](size_t i) { return y[i]; };
	matfreeApply(S, xo, yo);
}

}

extern "C" {

int fvhip_steady_backward_euler_device(fvhip_handle h, double* d_u, const fvhip_implicit_config* cfg,
                                       fvhip_solve_stats* stats, double* reshistory)
{
	return guard([&] {
		need(h, "handle");
		need(d_u, "u");
		if(!cfg || !stats) throw std::invalid_argument("null argument");
		System S = single(h);
		backwardEuler(S, {d_u}, *cfg, stats, reshistory);
		S.sync();
	});
}

int fvhip_group_steady_backward_euler_device(fvhip_group g, double* const* d_u, const fvhip_implicit_config* cfg,
                                             fvhip_solve_stats* stats, double* reshistory)
{
	return guard([&] {
		need(g, "group");
		needEach(d_u, g->hs.size(), "u");
		if(!cfg || !stats) throw std::invalid_argument("null argument");
		System S = ofGroup(g);
		backwardEuler(S, std::vector<double*>(d_u, d_u + S.size()), *cfg, stats, reshistory);
		S.sync();
	});
}

int fvhip_steady_forward_euler_device(fvhip_handle h, double* d_u, double cfl, double tol, int maxiter,
                                      int* steps, double* resratio, double* reshistory)
{
	return guard([&] {
		need(h, "handle");
		need(d_u, "u");
		System S = single(h);
		forwardEuler(S, {d_u}, cfl, tol, maxiter, steps, resratio, reshistory);
		S.sync();
	});
}

int fvhip_group_steady_forward_euler_device(fvhip_group g, double* const* d_u, double cfl, double tol, int maxiter,
                                            int* steps, double* resratio, double* reshistory)
{
	return guard([&] {
		need(g, "group");
		needEach(d_u, g->hs.size(), "u");
		System S = ofGroup(g);
		forwardEuler(S, std::vector<double*>(d_u, d_u + S.size()), cfl, tol, maxiter, steps, resratio, reshistory);
		S.sync();
	});
}

int fvhip_tvdrk_device(fvhip_handle h, double* d_u, int order, double cfl, double finaltime, int maxsteps,
                       int* steps, double* time)
{
	return guard([&] {
		need(h, "handle");
		need(d_u, "u");
		System S = single(h);
		tvdrk(S, {d_u}, order, cfl, finaltime, maxsteps, steps, time);
		S.sync();
	});
}

int fvhip_group_tvdrk_device(fvhip_group g, double* const* d_u, int order, double cfl, double finaltime, int maxsteps,
                             int* steps, double* time)
{
	return guard([&] {
		need(g, "group");
		needEach(d_u, g->hs.size(), "u");
		System S = ofGroup(g);
		tvdrk(S, std::vector<double*>(d_u, d_u + S.size()), order, cfl, finaltime, maxsteps, steps, time);
		S.sync();
	});
}

int fvhip_gmres_blocks_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                              const double* d_b, double* d_x, double rtol, int maxit, int restart, int sweeps,
                              int* iters, double* resnorm)
{
	return guard([&] {
		need(h, "handle");
		need(d_diag, "diag"); if(h->L.ninface > 0) { need(d_lower, "lower"); need(d_upper, "upper"); } need(d_b, "b"); need(d_x, "x");
		if(restart < 1 || restart > KRY_MAXK) throw std::invalid_argument("restart must be in [1, 128]");
		if(sweeps < 1) throw std::invalid_argument("sweeps must be >= 1");
		System S = single(h);
		h->ensureImplicit(restart);
		LinOp A{S};
		A.sweeps = sweeps;
		A.D = {d_diag}; A.Lo = {d_lower}; A.Up = {d_upper};
		A.setup();
		// the standalone solver keeps the selective reorthogonalisation it was pinned with (cgs_refine 1)
		const GmresOut g = gmres(S, A, [&](size_t) { return const_cast<double*>(d_b); },
		                         [&](size_t) { return d_x; }, rtol, maxit, restart, 1);
		S.sync();
		if(iters) *iters = g.iters;
		if(resnorm) *resnorm = g.rnorm;
	});
}

int fvhip_line_precondition_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                   double line_threshold, int single, const double* d_v, double* d_z)
{
	return guard([&] {
		need(h, "handle");
		need(d_diag, "diag"); if(h->L.ninface > 0) { need(d_lower, "lower"); need(d_upper, "upper"); } need(d_v, "v"); need(d_z, "z");
		if(!d_diag || !d_v || !d_z || (h->L.ninface > 0 && (!d_lower || !d_upper))) throw std::invalid_argument("null argument");
		HC(hipSetDevice(h->device));
		h->ensureLines(line_threshold);
		h->lines.single = single != 0;
		launch_line_factor(h->lines, d_diag, d_lower, d_upper, h->stream);
		launch_line_solve(h->lines, d_v, d_z, h->stream);
		HC(hipGetLastError());
		HC(hipStreamSynchronize(h->stream));
	});
}

int fvhip_ilu_precondition_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                  const double* d_v, double* d_z)
{
	return guard([&] {
		need(h, "handle");
		need(d_diag, "diag"); if(h->L.ninface > 0) { need(d_lower, "lower"); need(d_upper, "upper"); } need(d_v, "v"); need(d_z, "z");
		if(!d_diag || !d_v || !d_z || (h->L.ninface > 0 && (!d_lower || !d_upper))) throw std::invalid_argument("null argument");
		System S = single(h);
		h->ensureImplicit(1);
		LinOp A{S};
		A.ilu = true;
		A.D = {d_diag}; A.Lo = {d_lower}; A.Up = {d_upper};
		A.setup();
		A.precondition([&](size_t) { return const_cast<double*>(d_v); }, [&](size_t) { return d_z; });
		HC(hipGetLastError());
		S.sync();
	});
}

int fvhip_ilu_sweeps_precondition_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                                         int order, int build_sweeps, int apply_sweeps, int single, const double* d_v,
                                         double* d_z)
{
	return guard([&] {
		need(h, "handle");
		need(d_diag, "diag"); if(h->L.ninface > 0) { need(d_lower, "lower"); need(d_upper, "upper"); } need(d_v, "v"); need(d_z, "z");
		checkIluSweeps(order, build_sweeps, apply_sweeps, true);
		if(order == 0) throw std::invalid_argument("ilu_order must be 1 (internal order) or 2 (reverse Cuthill-McKee)");
		// ghost rows are neither read nor written (block-Jacobi across ranks), so a rank's handle needs neither its
		// communicator nor its group here
		System S{{h}, {}};
		HC(hipSetDevice(h->device));
		h->ensureImplicit(1);
		LinOp A{S};
		A.ilu = true; A.single = single != 0;
		A.ilu_order = order; A.ilu_build = build_sweeps; A.ilu_apply = apply_sweeps;
		A.D = {d_diag}; A.Lo = {d_lower}; A.Up = {d_upper};
		A.setup();
		A.precondition([&](size_t) { return const_cast<double*>(d_v); }, [&](size_t) { return d_z; });
		HC(hipGetLastError());
		S.sync();
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
		need(d_diag, "diag"); if(h->L.ninface > 0) { need(d_lower, "lower"); need(d_upper, "upper"); }
		if(levels < 2 || sweeps < 1 || coarse_sweeps < 1) throw std::invalid_argument("levels >= 2, sweeps >= 1, coarse_sweeps >= 1");
		if((d_v == nullptr) != (d_z == nullptr)) throw std::invalid_argument("v and z go together");
		if(smoother != 0 && smoother != 1) throw std::invalid_argument("smoother must be 0 or 1");
		const int rows = amgBlockRows(block_rows);
		System S = single(h);
		h->ensureImplicit(1);
		LinOp A{S};
		A.amg = levels; A.amg_sweeps = A.amg_fine = sweeps; A.amg_coarse = coarse_sweeps; A.amg_thr = threshold;
		A.amg_smoother = smoother; A.amg_rows = rows;
		A.lines = line_threshold > 0.0; A.line_thr = line_threshold;
		A.D = {d_diag}; A.Lo = {d_lower}; A.Up = {d_upper};
		A.setup();
		if(d_v) {
			// z needs ghost rows for the finest residuals: the handle's own operand buffer
			A.precondition([&](size_t) { return const_cast<double*>(d_v); }, [&](size_t) { return h->iw.z; });
			HC(hipMemcpyAsync(d_z, h->iw.z, 4*sizeof(double)*static_cast<size_t>(h->L.ncell), hipMemcpyDeviceToDevice, h->stream));
		}
		HC(hipGetLastError());
		S.sync();
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
		if(levels < 2 || sweeps < 1 || coarse_sweeps < 1) throw std::invalid_argument("levels >= 2, sweeps >= 1, coarse_sweeps >= 1");
		if((d_v == nullptr) != (d_z == nullptr)) throw std::invalid_argument("v and z go together");
		if(d_v) { needEach(d_v, n, "v"); needEach(d_z, n, "z"); }
		if(smoother != 0 && smoother != 1) throw std::invalid_argument("smoother must be 0 or 1");
		const int rows = amgBlockRows(block_rows);
		System S = ofGroup(g);
		S.each([&](size_t, fvhip_ctx* h) { h->ensureImplicit(1); });
		LinOp A{S};
		A.amg = levels; A.amg_sweeps = A.amg_fine = sweeps; A.amg_coarse = coarse_sweeps; A.amg_thr = threshold;
		A.amg_smoother = smoother; A.amg_rows = rows;
		A.lines = line_threshold > 0.0; A.line_thr = line_threshold;
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
		if(nlevels) for(size_t i = 0; i < n; i++) nlevels[i] = static_cast<int>(S.hs[i]->amg.size());
	});
}

int fvhip_amg_level(fvhip_handle h, int level, int* n, int* nnz, int* agg, int* rowptr, int* col, double* val)
{
	return guard([&] {
		need(h, "handle");
		if(level < 1 || level > static_cast<int>(h->amg.size())) throw std::invalid_argument("no such multigrid level");
		const AmgLevel& L = h->amg[static_cast<size_t>(level) - 1];
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

static AmgLevel& amgLevelOf(fvhip_handle h, int level)
{
	need(h, "handle");
	if(level < 1 || level > static_cast<int>(h->amg.size())) throw std::invalid_argument("no such multigrid level");
	return h->amg[static_cast<size_t>(level) - 1];
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
		const size_t bytes = 4*sizeof(double)*static_cast<size_t>(C.n);
		if(smoother == 1) {
			const int R = amgBlockRows(block_rows);
			if(!zero) HC(hipMemcpyAsync(C.x, d_x, bytes, hipMemcpyDeviceToDevice, h->stream));
			amgBlockSweeps(h, C, R, d_b, sweeps, direction, zero != 0);
			HC(hipMemcpyAsync(d_x, C.x, bytes, hipMemcpyDeviceToDevice, h->stream));
		} else if(C.n <= AMG_BLOCK_ROWS) {
			launch_amg_gs_block(C, d_b, d_x, sweeps, direction == 0, direction == 2, zero != 0, h->stream);
		} else {
			if(zero) exact::launch_fill(d_x, 0.0, 4LL*C.n, h->stream);
			const int nc = static_cast<int>(C.cstart_colour.size()) - 1;
			for(int k = 0; k < sweeps; k++) {
				const bool fwd = direction == 2 ? k % 2 == 0 : direction == 0;
				for(int q = 0; q < nc; q++) launch_amg_gs_colour(C, fwd ? q : nc - 1 - q, d_b, d_x, h->stream);
			}
		}
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
