/** \file implicit.cpp
 * \brief Device-resident pseudo-time solvers over one global system:
 *   SteadyForwardEulerSolver::solve (aodesolver.cpp:135-282) and SteadyBackwardEulerSolver::solve
 *   (aodesolver.cpp:363-638), plus the matrix-free operator over a system.
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

/// SteadyForwardEulerSolver::solve (aodesolver.cpp:135-282): u += cflinit dtm/area r (the ramped
/// CFL is only reported by the reference, :194, :208)
static void forwardEuler(System& S, const std::vector<double*>& us, double cfl, double tol, int maxiter,
                         int* steps, double* resratio, double* hist)
{
	S.each([&](size_t, fvhip_ctx* h) { h->ensureReductions(); });
	double resi = 1.0, initres = 1.0;
	int step = 0;
	while(resi/initres > tol && step < maxiter) {
		S.residual(us);                                                                           // :180-189
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
	int step = 0;
	double time = 0;
	while(time <= finaltime - 1e-12 && step < maxsteps) {
		S.residual(us);                                                             // :712-719 (zeroed, -r(u))
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

/// the time-accurate driver's arguments, refused by name before any handle or device is touched
static void checkUnsteady(const fvhip_unsteady_config* c, const fvhip_unsteady_stats* st)
{
	need(c, "config");
	need(st, "stats");
	if(c->order < 1 || c->order > 3) throw std::invalid_argument("SSP-RK: temporal order must be 1, 2 or 3");
	if(c->maxsteps < 1) throw std::invalid_argument("SSP-RK: maxsteps must be >= 1");
	if(!(c->finaltime > 0.0)) throw std::invalid_argument("SSP-RK: finaltime must be > 0");
	if((c->cfl > 0.0) == (c->dt > 0.0))
		throw std::invalid_argument("SSP-RK: exactly one of cfl > 0 and dt > 0 must be given");
}

/// Time-accurate Shu-Osher SSP Runge-Kutta of order 1-3 (the coefficients of initialize_TVDRK_Coeffs,
/// aodesolver.cpp:45-67). Unlike tvdrk above, which keeps the reference's loop as written, every stage's residual
/// is taken at that stage's state (tvdrk: at the step's start state, which makes every order forward Euler), the
/// update adds the assembled residual (d_r holds -r(u), so u' = -r/area is u += h/area d_r; tvdrk keeps the
/// reference's minus and runs backwards in time) and the last step is shortened to land on finaltime exactly.
/// Per step: d_r, d_dtm at u; dtmin = global minimum of d_dtm (read every step: the divergence check and
/// cfl_max = max h/dtmin); h = dt if given, else cfl dtmin, cut to finaltime - t when t + h reaches finaltime;
/// stage s: ustage = (c0 u + c1 ustage) + ((c2 h)/area) d_r with d_r at ustage for s >= 2; the last stage
/// writes u. The stage state is a residual's input (its ghost rows get filled), hence d_sspstage with ghost rows.
/// record [maxsteps][6] (host, may be null): t after the step, h, and sum area u of the four conserved variables.
static void ssprk(System& S, const std::vector<double*>& us, const fvhip_unsteady_config& c, fvhip_unsteady_stats* st,
                  double* record)
{
	static const double coef[3][3][3] = {                                       // initialize_TVDRK_Coeffs :45-67
		{{1.0, 0.0, 1.0}, {0, 0, 0}, {0, 0, 0}},
		{{1.0, 0.0, 1.0}, {0.5, 0.5, 0.5}, {0, 0, 0}},
		{{1.0, 0.0, 1.0}, {0.75, 0.25, 0.25}, {0.3333333333333333, 0.6666666666666667, 0.6666666666666667}}};
	const double (*tc)[3] = coef[c.order-1];
	std::vector<double*> ust;
	S.each([&](size_t, fvhip_ctx* h) {
		h->ensureReductions();
		if(!h->d_sspstage) h->d_sspstage = dalloc(4*static_cast<size_t>(std::max(h->ntotal(), 1)), h->owned);
		ust.push_back(h->d_sspstage);
	});
	int step = 0;
	double time = 0, hmin = INFINITY, hmax = 0, cflmax = 0;
	while(time < c.finaltime && step < c.maxsteps) {
		S.residual(us);                                                             // -r(u^n), local time steps
		S.each([&](size_t, fvhip_ctx* h) {
			launch_min(h->L.ncell, h->d_dtm, h->iw.part, h->iw.red, h->stream);
			if(h->comm) NC(ncclAllReduce(h->iw.red, h->iw.red, 1, ncclDouble, ncclMin, h->comm, h->stream));
			HC(hipMemcpyAsync(h->iw.h_red, h->iw.red, sizeof(double), hipMemcpyDeviceToHost, h->stream));
		});
		double dtmin = INFINITY;
		S.each([&](size_t, fvhip_ctx* h) { HC(hipStreamSynchronize(h->stream)); dtmin = std::min(dtmin, h->iw.h_red[0]); });
		if(!std::isfinite(dtmin)) throw std::runtime_error("SSP-RK diverged - dtmin is Nan or inf!");
		double dt = c.dt > 0.0 ? c.dt : c.cfl*dtmin;
		const bool last = time + dt >= c.finaltime;
		if(last) dt = c.finaltime - time;
		for(int s = 0; s < c.order; s++) {
			if(s > 0) S.residual(ust);                                              // -r at the stage state
			const double sc = tc[s][2]*dt;
			S.each([&](size_t i, fvhip_ctx* h) {
				// the first stage has c1 = 0 and reads u in ustage's place; the last writes u
				launch_ssprk_stage(h->L.ncell, tc[s][0], tc[s][1], sc, h->M.area, h->d_r, us[i], s == 0 ? us[i] : ust[i],
				                   s == c.order-1 ? us[i] : ust[i], h->stream);
				HC(hipGetLastError());
			});
		}
		time = last ? c.finaltime : time + dt;
		hmin = std::min(hmin, dt); hmax = std::max(hmax, dt); cflmax = std::max(cflmax, dt/dtmin);
		if(record) {
			S.each([&](size_t i, fvhip_ctx* h) {
				launch_conserved(h->L.ncell, us[i], h->M.area, h->iw.part, h->iw.red, h->stream);
				HC(hipGetLastError());
			});
			const std::vector<double> sums = S.allsum(4, false);
			double* row = record + 6*static_cast<size_t>(step);
			row[0] = time; row[1] = dt;
			std::copy(sums.begin(), sums.end(), row + 2);
		}
		step++;
	}
	st->steps = step;
	st->time = time;
	st->dt_min = hmin; st->dt_max = hmax; st->cfl_max = cflmax;
}

typedef std::vector<double*> States;

/// a stepper's entry point on one handle / on a group: the arguments checked (have: its other pointers are there),
/// the system made, `step(S, states)` run and waited for
template <typename F> static int onHandle(fvhip_handle h, double* d_u, bool have, F&& step)
{
	return guard([&] {
		need(h, "handle");
		need(d_u, "u");
		if(!have) throw std::invalid_argument("null argument");
		System S = single(h);
		step(S, States{d_u});
		S.sync();
	});
}
template <typename F> static int onGroup(fvhip_group g, double* const* d_u, bool have, F&& step)
{
	return guard([&] {
		need(g, "group");
		needEach(d_u, g->hs.size(), "u");
		if(!have) throw std::invalid_argument("null argument");
		System S = ofGroup(g);
		step(S, States(d_u, d_u + S.size()));
		S.sync();
	});
}

}

using namespace fvhip_detail;

extern "C" {

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

int fvhip_steady_forward_euler_device(fvhip_handle h, double* d_u, double cfl, double tol, int maxiter,
                                      int* steps, double* resratio, double* reshistory)
{
	return onHandle(h, d_u, true, [&](System& S, const States& us) { forwardEuler(S, us, cfl, tol, maxiter, steps, resratio, reshistory); });
}

int fvhip_group_steady_forward_euler_device(fvhip_group g, double* const* d_u, double cfl, double tol, int maxiter,
                                            int* steps, double* resratio, double* reshistory)
{
	return onGroup(g, d_u, true, [&](System& S, const States& us) { forwardEuler(S, us, cfl, tol, maxiter, steps, resratio, reshistory); });
}

int fvhip_tvdrk_device(fvhip_handle h, double* d_u, int order, double cfl, double finaltime, int maxsteps,
                       int* steps, double* time)
{
	return onHandle(h, d_u, true, [&](System& S, const States& us) { tvdrk(S, us, order, cfl, finaltime, maxsteps, steps, time); });
}

int fvhip_group_tvdrk_device(fvhip_group g, double* const* d_u, int order, double cfl, double finaltime, int maxsteps,
                             int* steps, double* time)
{
	return onGroup(g, d_u, true, [&](System& S, const States& us) { tvdrk(S, us, order, cfl, finaltime, maxsteps, steps, time); });
}

int fvhip_ssprk_device(fvhip_handle h, double* d_u, const fvhip_unsteady_config* cfg, fvhip_unsteady_stats* stats,
                       double* record)
{
	if(guard([&] { checkUnsteady(cfg, stats); })) return 1;
	return onHandle(h, d_u, true, [&](System& S, const States& us) { ssprk(S, us, *cfg, stats, record); });
}

int fvhip_group_ssprk_device(fvhip_group g, double* const* d_u, const fvhip_unsteady_config* cfg,
                             fvhip_unsteady_stats* stats, double* record)
{
	if(guard([&] { checkUnsteady(cfg, stats); })) return 1;
	return onGroup(g, d_u, true, [&](System& S, const States& us) { ssprk(S, us, *cfg, stats, record); });
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
