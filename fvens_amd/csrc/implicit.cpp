/** \file implicit.cpp
 * \brief The device-resident implicit pseudo-time solver over one global system:
 *   SteadyBackwardEulerSolver::solve (aodesolver.cpp:363-638), its GMRES and the matrix-free operator over a
 *   system, and the implicit time-accurate driver round the same iteration (dualTime: BDF1/BDF2 in dual time).
 *   The explicit drivers are in explicit.cpp.
 *
 * The reference hands each linear system to PETSc (KSPSolve, aodesolver.cpp:483; GMRES with a
 * block-Jacobi/ILU or SOR preconditioner from the .solverc files). Here it is solved on the device
 * by restarted GMRES: right-preconditioned (the residual it monitors is the true one), classical
 * Gram-Schmidt with selective (DGKS) re-orthogonalisation (one fused multi-dot reduction, i.e. one
 * small host round trip, per Arnoldi step in the common case, a second only when the projection
 * cancelled more than half of |w|^2; modified Gram-Schmidt would take j+1), preconditioned by
 * block-Jacobi sweeps on the assembled first-order Jacobian (precond.cpp; the options: precond_options.hpp).
 * PETSc's ILU/SOR are sequential recurrences; a block-Jacobi sweep is one launch over all cells, and
 * several sweeps approach the block Gauss-Seidel effect. The matrix-free operator (alinalg.cpp:142-233)
 * uses the assembled blocks as preconditioner, as the reference's KSPSetOperators(A_mf, M) does
 * (casesolvers.cpp:170).
 *
 * A system (system.hpp) is either one handle (one GPU, or one rank of a partition with its RCCL communicator:
 * partial sums combined by ncclAllReduce) or all ranks of a partition driven from one process (a
 * group: halo rows by device copies, partial sums added on the host in handle order).
 */
#include "linop.hpp"

#include <cmath>
#include <vector>

namespace fvhip_detail {

/// the perturbed state gets its ghost rows from the residual's own exchange
void matfreeApply(System& S, const ArrayOf& x, const ArrayOf& y, bool have_norm)
{
	S.each([&](size_t i, fvhip_ctx* h) {
		if(!h->mf_u || !h->mf_r || !h->mf_mdt) throw std::runtime_error("matrix-free operator: state not set");
		if(!have_norm) launch_mdot(4LL*h->L.ncell, 0, nullptr, 0, x(i), true, h->iw.part, h->iw.red, h->stream);
	});
	if(!have_norm) S.allsumDevice(1);          // |x|^2 stays on the device (launch_pertmag reads it there)
	if(S.size() == 1 && !S.legs && S.hs[0]->matfreeFusable() && S.hs[0]->matfreeNoAlias(S.hs[0]->mf_u, x(0), y(0))) {
		// one launch: the perturbed state and the combination inside the residual kernel (bitwise the same)
		fvhip_ctx* h = S.hs[0];
		launch_pertmag(h->iw.red, h->mf_eps, h->iw.pm, h->stream);
		h->stage_fused(h->mf_u, y(0), false, nullptr, true, nullptr, 0, nullptr, MfFuse{x(0), h->iw.pm, h->mf_r, h->mf_mdt});
		return;
	}
	std::vector<double*> aux, yg, none(S.size(), nullptr);
	S.each([&](size_t i, fvhip_ctx* h) {
		launch_pertmag(h->iw.red, h->mf_eps, h->iw.pm, h->stream);
		launch_mf_perturb(4LL*h->L.ncell, h->mf_u, x(i), h->iw.pm, h->iw.aux, h->stream);
		aux.push_back(h->iw.aux);
		yg.push_back(h->iw.yg);
	});
	residual(S, aux.data(), yg.data(), false, none.data(), true);
	S.each([&](size_t i, fvhip_ctx* h) {
		launch_mf_combine(h->L.ncell, h->mf_mdt, x(i), h->iw.yg, h->mf_r, h->iw.pm, y(i), h->stream);
		HC(hipGetLastError());
	});
}

void LinOp::blocks(const ArrayOf& x, const ArrayOf& y) {
	S.exchange(x, 4);
	S.each([&](size_t i, fvhip_ctx* h) {
		h->timed("k_block_apply", [&]{ launch_block_apply(h->J, D[i], Lo[i], Up[i], x(i), y(i), h->stream); });
	});
}

void LinOp::apply(const ArrayOf& x, const ArrayOf& y) {
	const bool have = znorm;
	znorm = false;
	if(o.matfree) matfreeApply(S, x, y, have);
	else blocks(x, y);
}

/// Restarted GMRES(m) for A x = b, x0 = 0; stops when |b - A x| <= rtol |b| or after maxit
/// Arnoldi steps in total (KSPSolve with -ksp_rtol, -ksp_max_it, -ksp_gmres_restart). refine: cgs_refine, 0 to 2
static GmresOut gmres(System& S, LinOp& A, const ArrayOf& b, const ArrayOf& x, double rtol, int maxit, int m,
                      int refine = 0)
{
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
	/// projects w on V(0..j): the coefficients h = V^T w summed over the system, returned on the host (with_norm:
	/// |w|^2 after them) and left in every handle's iw.red; column j of H is set to them, or has them added
	auto project = [&](int j, bool with_norm, bool add) {
		S.each([&](size_t i, fvhip_ctx* h) {
			launch_mdot(n4(i), j+1, V(i,0), n4(i), w(i), with_norm, h->iw.part, h->iw.red, h->stream);
		});
		const std::vector<double> hj = S.allsum(j + (with_norm ? 2 : 1), true);
		for(int k = 0; k <= j; k++) Hij(k,j) = add ? Hij(k,j) + hj[k] : hj[k];
		return hj;
	};
	/// w -= V(0..j) h with the coefficients in iw.red
	auto subtract = [&](int j) {
		S.each([&](size_t i, fvhip_ctx* h) { launch_maxpy(n4(i), j+1, V(i,0), n4(i), h->iw.red, w(i), h->stream); });
	};
	/// |w|^2 - |h|^2 of a projection that returned both: |w - V h|^2 by Pythagoras
	auto remaining = [&](const std::vector<double>& hj, int j) {
		double corr = 0.0;
		for(int k = 0; k <= j; k++) corr += hj[k]*hj[k];
		return hj[j+1] - corr;
	};
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
				project(j, false, false);
				if(refine == 2) { subtract(j); project(j, false, true); }
				S.each([&](size_t i, fvhip_ctx* h) {
					launch_maxpy_norm(n4(i), j+1, V(i,0), n4(i), h->iw.red, w(i), h->iw.part, h->iw.red, h->stream);
				});
				hn2 = S.allsum(1, false)[0];
			} else {
				const std::vector<double> h1 = project(j, true, false);
				subtract(j);
				hn2 = remaining(h1, j);
				if(!(hn2 > 0.5*h1[j+1])) {
					const std::vector<double> h2 = project(j, true, true);
					subtract(j);
					hn2 = remaining(h2, j);
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

/// SteadyBackwardEulerSolver::solve (aodesolver.cpp:363-638) on device states us (internal order,
/// ghost rows included on partitioned handles)
static void backwardEuler(System& S, const std::vector<double*>& us, const fvhip_implicit_config& c,
                          fvhip_solve_stats* st, double* hist)
{
	LinOp A{S, PrecondOptions::of(c)};
	A.o.check();
	S.each([&](size_t, fvhip_ctx* h) { h->ensureImplicit(c.restart); h->mf_eps = c.mf_eps; });
	for(fvhip_ctx* h : S.hs) { A.D.push_back(h->iw.jd); A.Lo.push_back(h->iw.jlo); A.Up.push_back(h->iw.jup); }
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
		S.residual(us);              // r = 0 + (-r(u)) with local time steps (:421-452)
		curCFL = expResidualRamp(c.cflinit, c.cflfin, curCFL, resiold/resi, 0.25, 0.3);           // :462
		// Jacobian (:456-457) with the pseudo-time term (:467) added in its diagonal pass
		S.each([&](size_t i, fvhip_ctx* h) { h->assemble(us[i], h->iw.jd, h->iw.jlo, h->iw.jup, curCFL, h->d_dtm); });
		A.setup();
		if(A.o.matfree)                                                                             // :386-394
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
	if(A.o.matfree) S.each([&](size_t, fvhip_ctx* h) { h->mf_u = h->mf_r = h->mf_mdt = nullptr; });
	st->steps = step;
	st->lin_iters = lin;
	st->resratio = resi/initres;
	st->converged = (step < c.maxiter && resi/initres <= c.tol) ? 1 : 0;                            // :618-632
	st->cfl = curCFL;
	st->lin_unconverged = linbad;
	st->lin_worst = linworst;
}

/// a step that would end within this fraction of itself before finaltime is stretched to land on it (dualTime)
static const double BDF_SLIVER = 1e-9;

/// the dual-time driver's arguments, refused by name before any handle or device is touched
static void checkDualTime(const fvhip_unsteady_config* c, const fvhip_implicit_config* ic, const fvhip_unsteady_stats* st,
                          const fvhip_dualtime_stats* ds)
{
	need(c, "config");
	need(ic, "implicit config");
	need(st, "stats");
	need(ds, "dual-time stats");
	if(c->order < 1 || c->order > 2) throw std::invalid_argument("BDF: temporal order must be 1 or 2");
	if(c->maxsteps < 1) throw std::invalid_argument("BDF: maxsteps must be >= 1");
	if(!(c->finaltime > 0.0)) throw std::invalid_argument("BDF: finaltime must be > 0");
	if((c->cfl > 0.0) == (c->dt > 0.0))
		throw std::invalid_argument("BDF: exactly one of cfl > 0 and dt > 0 must be given");
	if(ic->maxiter < 1) throw std::invalid_argument("BDF: maxiter (inner iterations per step) must be >= 1");
	if(ic->resume_res0 > 0.0 || ic->resume_res > 0.0 || ic->resume_res_prev > 0.0 || ic->resume_cfl > 0.0)
		throw std::invalid_argument("BDF: resume_* continues a steady solve; the inner iteration starts anew every step");
}

/// Implicit time-accurate stepping in dual time: BDF1, or BDF2 with variable step (its first step is BDF1).
/// d_r = -r(u) as the residual leaves it, so area du/dt = d_r and one physical step of size h finds u with
///   G(u) = d_r(u) - (area/h)*((a0*u + a1*u^n) + a2*u^(n-1)) = 0          (k_bdf_residual, ode.hip)
/// BDF1: a = (1, -1, 0). BDF2 with w = h/h_prev: a0 = (1+2w)/(1+w), a1 = -(1+w), a2 = w^2/(1+w).
/// G = 0 is solved by backwardEuler's pseudo-time iteration applied to G, from u = u^n: per inner iteration
///   [(m + s area) I + dr/du] du = G(u),   m = area/(cfl_tau dtm),  s = a0/h
/// which is the steady system with b = G and m + s area where it has m -- in the diagonal blocks and in d_dtm,
/// the matrix-free operator's mdt (k_bdf_time_term after the assembly). The matrix-free operator differences the
/// spatial residual, so d_r stays that and G has a buffer of its own.
/// Per step: d_r, d_dtm at u^n; dtmin as ssprk reads it; h = dt or cfl dtmin, set to finaltime - t when t + h
/// reaches finaltime or ends within BDF_SLIVER h of it (that step has w != 1). Then: G and g = sqrt(sum area sum_v G^2) at the current u; stop
/// when g <= tol g0 (g0: the step's first g; g0 == 0 leaves the state as it is) or after maxiter solves, else ramp
/// the pseudo CFL on g_old/g from cflinit, assemble, add the time term, set up the preconditioner, solve, update.
/// The test comes before the solve, so the returned state is the one whose G was measured.
/// record [maxsteps][8] (host, may be null): t after the step, h, inner iterations, final g/g0, sum area u.
static void dualTime(System& S, const std::vector<double*>& us, const fvhip_unsteady_config& c,
                     const fvhip_implicit_config& ic, fvhip_unsteady_stats* st, fvhip_dualtime_stats* ds, double* record)
{
	LinOp A{S, PrecondOptions::of(ic)};
	A.o.check();
	S.each([&](size_t, fvhip_ctx* h) {
		h->ensureImplicit(ic.restart);
		h->mf_eps = ic.mf_eps;
		if(!h->d_bdf_g) {
			const size_t n4 = 4*static_cast<size_t>(h->L.ncell);
			h->d_bdf_n = dalloc(n4, h->owned); h->d_bdf_m = dalloc(n4, h->owned); h->d_bdf_g = dalloc(n4, h->owned);
		}
	});
	for(fvhip_ctx* h : S.hs) { A.D.push_back(h->iw.jd); A.Lo.push_back(h->iw.jlo); A.Up.push_back(h->iw.jup); }
	const ArrayOf bs = [&](size_t i) { return S.hs[i]->d_bdf_g; };
	const ArrayOf xs = [&](size_t i) { return S.hs[i]->iw.du; };
	const char* diverged = "BDF dual time diverged - residual is Nan or inf!";

	int step = 0;
	double time = 0, hprev = 0, hmin = INFINITY, hmax = 0, cflmax = 0;
	*ds = fvhip_dualtime_stats{};
	while(time < c.finaltime && step < c.maxsteps) {
		S.each([&](size_t i, fvhip_ctx* h) {                                    // u^(n-1) <- u^n, u^n <- u
			std::swap(h->d_bdf_n, h->d_bdf_m);
			HC(hipMemcpyAsync(h->d_bdf_n, us[i], sizeof(double)*4*static_cast<size_t>(h->L.ncell),
			                  hipMemcpyDeviceToDevice, h->stream));
		});
		S.residual(us);                                                         // -r(u^n), local time steps
		const double dtmin = S.allmin();
		if(!std::isfinite(dtmin)) throw std::runtime_error(diverged);           // a NaN state: its time step is NaN
		double dt = c.dt > 0.0 ? c.dt : c.cfl*dtmin;
		// the last step: ssprk's test, and also when the step would leave a remainder of rounding size (ten steps of
		// 0.2 sum to 2 - 2^-52). A step of that size has w ~ 1e-15, and the rounding of a0 + a1 times u/h is O(1) in G
		const bool last = time + dt >= c.finaltime || c.finaltime - (time + dt) <= BDF_SLIVER*dt;
		if(last) dt = c.finaltime - time;
		double a0 = 1.0, a1 = -1.0, a2 = 0.0;
		if(c.order == 2 && step > 0) {
			const double w = dt/hprev;
			a0 = (1.0 + 2.0*w)/(1.0 + w); a1 = -(1.0 + w); a2 = w*w/(1.0 + w);
		}
		const double s = a0/dt;

		double g = 0, g0 = 0, gold = 0, curCFL = 0;
		int k = 0;
		while(true) {
			if(k > 0) S.residual(us);
			S.each([&](size_t i, fvhip_ctx* h) {
				launch_bdf_residual(h->L.ncell, a0, a1, a2, dt, h->M.area, h->d_r, us[i], h->d_bdf_n,
				                    a2 != 0.0 ? h->d_bdf_m : nullptr, h->d_bdf_g, h->iw.part, h->iw.red, h->stream);
				HC(hipGetLastError());
			});
			gold = g;
			g = std::sqrt(S.allsum(1, false)[0]);
			if(!std::isfinite(g)) throw std::runtime_error(diverged);
			if(k == 0) { g0 = gold = g; if(g0 == 0.0) break; }
			if(g <= ic.tol*g0 || k >= ic.maxiter) break;
			curCFL = expResidualRamp(ic.cflinit, ic.cflfin, curCFL, gold/g, 0.25, 0.3);
			S.each([&](size_t i, fvhip_ctx* h) {
				h->assemble(us[i], h->iw.jd, h->iw.jlo, h->iw.jup, curCFL, h->d_dtm);
				h->timed("k_bdf_time_term", [&]{ launch_bdf_time_term(h->L.ncell, s, h->M.area, h->d_dtm, h->iw.jd, h->stream); });
				HC(hipGetLastError());
			});
			A.setup();
			if(A.o.matfree)
				S.each([&](size_t i, fvhip_ctx* h) { h->mf_u = us[i]; h->mf_r = h->d_r; h->mf_mdt = h->d_dtm; });
			const GmresOut lin = gmres(S, A, bs, xs, ic.lin_rtol, ic.lin_maxit, ic.restart, ic.cgs_refine);
			ds->lin_iters += lin.iters;
			if(lin.rnorm0 > 0.0 && lin.rnorm > ic.lin_rtol*lin.rnorm0) ds->lin_unconverged++;
			S.each([&](size_t i, fvhip_ctx* h) {
				launch_relaxed_update(h->L.ncell, h->P.gas, ic.min_relax, h->iw.du, us[i], h->stream);
				HC(hipGetLastError());
			});
			k++;
		}
		const double ratio = g0 > 0.0 ? g/g0 : 0.0;
		ds->inner_iters += k;
		ds->inner_max = std::max(ds->inner_max, k);
		if(g0 > 0.0 && g > ic.tol*g0) ds->inner_unconverged++;
		ds->worst_ratio = std::max(ds->worst_ratio, ratio);

		time = last ? c.finaltime : time + dt;
		hprev = dt;
		hmin = std::min(hmin, dt); hmax = std::max(hmax, dt); cflmax = std::max(cflmax, dt/dtmin);
		if(record) {
			S.each([&](size_t i, fvhip_ctx* h) {
				launch_conserved(h->L.ncell, us[i], h->M.area, h->iw.part, h->iw.red, h->stream);
				HC(hipGetLastError());
			});
			const std::vector<double> sums = S.allsum(4, false);
			double* row = record + 8*static_cast<size_t>(step);
			row[0] = time; row[1] = dt; row[2] = k; row[3] = ratio;
			std::copy(sums.begin(), sums.end(), row + 4);
		}
		step++;
	}
	if(A.o.matfree) S.each([&](size_t, fvhip_ctx* h) { h->mf_u = h->mf_r = h->mf_mdt = nullptr; });
	st->steps = step;
	st->time = time;
	st->dt_min = hmin; st->dt_max = hmax; st->cfl_max = cflmax;
}

}

using namespace fvhip_detail;

extern "C" {

int fvhip_bdf_device(fvhip_handle h, double* d_u, const fvhip_unsteady_config* cfg, const fvhip_implicit_config* icfg,
                     fvhip_unsteady_stats* stats, fvhip_dualtime_stats* dstats, double* record)
{
	if(guard([&] { checkDualTime(cfg, icfg, stats, dstats); })) return 1;
	return onHandle(h, d_u, true, [&](System& S, const States& us) { dualTime(S, us, *cfg, *icfg, stats, dstats, record); });
}

int fvhip_group_bdf_device(fvhip_group g, double* const* d_u, const fvhip_unsteady_config* cfg,
                           const fvhip_implicit_config* icfg, fvhip_unsteady_stats* stats, fvhip_dualtime_stats* dstats,
                           double* record)
{
	if(guard([&] { checkDualTime(cfg, icfg, stats, dstats); })) return 1;
	return onGroup(g, d_u, true, [&](System& S, const States& us) { dualTime(S, us, *cfg, *icfg, stats, dstats, record); });
}

int fvhip_bdf_residual_device(fvhip_handle h, double* d_u, const double* d_un, const double* d_um, double a0, double a1,
                              double a2, double hstep, double* d_g, double* sumsq)
{
	if(guard([&] {
		need(d_un, "un"); need(d_g, "g"); need(sumsq, "sumsq");
		if(a2 != 0.0) need(d_um, "um");
		if(!(hstep > 0.0)) throw std::invalid_argument("BDF residual: the step must be > 0");
	})) return 1;
	return onHandle(h, d_u, true, [&](System& S, const States& us) {
		h->ensureReductions();
		S.residual(us);
		launch_bdf_residual(h->L.ncell, a0, a1, a2, hstep, h->M.area, h->d_r, d_u, d_un, a2 != 0.0 ? d_um : nullptr, d_g,
		                    h->iw.part, h->iw.red, h->stream);
		HC(hipGetLastError());
		*sumsq = S.allsum(1, false)[0];
	});
}

int fvhip_steady_backward_euler_device(fvhip_handle h, double* d_u, const fvhip_implicit_config* cfg,
                                       fvhip_solve_stats* stats, double* reshistory)
{
	return onHandle(h, d_u, cfg && stats, [&](System& S, const States& us) { backwardEuler(S, us, *cfg, stats, reshistory); });
}

int fvhip_group_steady_backward_euler_device(fvhip_group g, double* const* d_u, const fvhip_implicit_config* cfg,
                                             fvhip_solve_stats* stats, double* reshistory)
{
	return onGroup(g, d_u, cfg && stats, [&](System& S, const States& us) { backwardEuler(S, us, *cfg, stats, reshistory); });
}

int fvhip_gmres_blocks_device(fvhip_handle h, const double* d_diag, const double* d_lower, const double* d_upper,
                              const double* d_b, double* d_x, double rtol, int maxit, int restart, int sweeps,
                              int* iters, double* resnorm)
{
	return guard([&] {
		need(h, "handle");
		needBlocks(h->L.ninface, d_diag, d_lower, d_upper); need(d_b, "b"); need(d_x, "x");
		if(restart < 1 || restart > KRY_MAXK) throw std::invalid_argument("restart must be in [1, 128]");
		if(sweeps < 1) throw std::invalid_argument("sweeps must be >= 1");
		System S = single(h);
		h->ensureImplicit(restart);
		LinOp A{S};
		// the standalone solver keeps the selective reorthogonalisation it was pinned with (cgs_refine 1)
		A.o.sweeps = sweeps; A.o.restart = restart; A.o.cgs_refine = 1;
		A.o.check();
		A.D = {d_diag}; A.Lo = {d_lower}; A.Up = {d_upper};
		A.setup();
		const GmresOut g = gmres(S, A, [&](size_t) { return const_cast<double*>(d_b); },
		                         [&](size_t) { return d_x; }, rtol, maxit, restart, A.o.cgs_refine);
		S.sync();
		if(iters) *iters = g.iters;
		if(resnorm) *resnorm = g.rnorm;
	});
}

}
