/** \file explicit.cpp
 * \brief Device-resident explicit drivers over one global system (system.hpp): SteadyForwardEulerSolver::solve
 *   (aodesolver.cpp:135-282), TVDRKSolver::solve (aodesolver.cpp:669-758) as the reference wrote it, and the
 *   time-accurate Shu-Osher SSP Runge-Kutta driver. Their kernels are in ode.hip.
 */
#include "system.hpp"

#include <cmath>
#include <vector>

namespace fvhip_detail {

/// Shu-Osher coefficients (c0, c1, c2) of stage s of the scheme of order o, SHU_OSHER[o-1][s]
/// (initialize_TVDRK_Coeffs, aodesolver.cpp:45-67): ustage = c0 u + c1 ustage + c2 h L(.)
static const double SHU_OSHER[3][3][3] = {
	{{1.0, 0.0, 1.0}, {0, 0, 0}, {0, 0, 0}},
	{{1.0, 0.0, 1.0}, {0.5, 0.5, 0.5}, {0, 0, 0}},
	{{1.0, 0.0, 1.0}, {0.75, 0.25, 0.25}, {0.3333333333333333, 0.6666666666666667, 0.6666666666666667}}};

/// every handle's reduction scratch and its one stage buffer d_stage (owned + ghost rows), returned per handle
static std::vector<double*> stageBuffers(System& S)
{
	std::vector<double*> ust;
	S.each([&](size_t, fvhip_ctx* h) {
		h->ensureReductions();
		if(!h->d_stage) h->d_stage = dalloc(4*static_cast<size_t>(std::max(h->ntotal(), 1)), h->owned);
		ust.push_back(h->d_stage);
	});
	return ust;
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
/// reused. The stage is launch_rk_stage with the negated sc = (c2 dtmin) cfl, in place on the owned rows of
/// d_stage: the subtraction as written, bit for bit (ode.hip k_rk_stage). maxsteps caps the loop (the reference
/// has no cap).
static void tvdrk(System& S, const std::vector<double*>& us, int order, double cfl, double finaltime, int maxsteps,
                  int* steps, double* time_out)
{
	if(order < 1 || order > 3) throw std::invalid_argument("TVD RK: temporal order must be 1, 2 or 3");
	if(maxsteps < 1) throw std::invalid_argument("TVD RK: maxsteps must be >= 1");
	const double (*tc)[3] = SHU_OSHER[order-1];
	const std::vector<double*> ust = stageBuffers(S);
	S.each([&](size_t i, fvhip_ctx* h) {
		HC(hipMemcpyAsync(ust[i], us[i], sizeof(double)*4*static_cast<size_t>(h->L.ncell), hipMemcpyDeviceToDevice,
		                  h->stream));
	});
	int step = 0;
	double time = 0;
	while(time <= finaltime - 1e-12 && step < maxsteps) {
		S.residual(us);                                                             // :712-719 (zeroed, -r(u))
		const double dtmin = S.allmin();
		if(!std::isfinite(dtmin)) throw std::runtime_error("TVDRK solver diverged - dtmin is Nan or inf!");   // :730-731
		for(int s = 0; s < order; s++) {
			const double sc = tc[s][2]*dtmin*cfl;
			S.each([&](size_t i, fvhip_ctx* h) {
				launch_rk_stage(h->L.ncell, tc[s][0], tc[s][1], -sc, h->M.area, h->d_r, us[i], ust[i], ust[i], h->stream);
			});
		}
		S.each([&](size_t i, fvhip_ctx* h) {
			HC(hipMemcpyAsync(us[i], ust[i], sizeof(double)*4*static_cast<size_t>(h->L.ncell), hipMemcpyDeviceToDevice,
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

/// Time-accurate Shu-Osher SSP Runge-Kutta of order 1-3. Unlike tvdrk above, which keeps the reference's loop as
/// written, every stage's residual is taken at that stage's state (tvdrk: at the step's start state, which makes
/// every order forward Euler), the update adds the assembled residual (d_r holds -r(u), so u' = -r/area is
/// u += h/area d_r; tvdrk keeps the reference's minus and runs backwards in time) and the last step is shortened
/// to land on finaltime exactly.
/// Per step: d_r, d_dtm at u; dtmin = global minimum of d_dtm (read every step: the divergence check and
/// cfl_max = max h/dtmin); h = dt if given, else cfl dtmin, cut to finaltime - t when t + h reaches finaltime;
/// stage s: ustage = (c0 u + c1 ustage) + ((c2 h)/area) d_r with d_r at ustage for s >= 2; the last stage
/// writes u. The stage state is a residual's input (its ghost rows get filled), hence d_stage's ghost rows.
/// record [maxsteps][6] (host, may be null): t after the step, h, and sum area u of the four conserved variables.
static void ssprk(System& S, const std::vector<double*>& us, const fvhip_unsteady_config& c, fvhip_unsteady_stats* st,
                  double* record)
{
	const double (*tc)[3] = SHU_OSHER[c.order-1];
	const std::vector<double*> ust = stageBuffers(S);
	int step = 0;
	double time = 0, hmin = INFINITY, hmax = 0, cflmax = 0;
	while(time < c.finaltime && step < c.maxsteps) {
		S.residual(us);                                                             // -r(u^n), local time steps
		const double dtmin = S.allmin();
		if(!std::isfinite(dtmin)) throw std::runtime_error("SSP-RK diverged - dtmin is Nan or inf!");
		double dt = c.dt > 0.0 ? c.dt : c.cfl*dtmin;
		const bool last = time + dt >= c.finaltime;
		if(last) dt = c.finaltime - time;
		for(int s = 0; s < c.order; s++) {
			if(s > 0) S.residual(ust);                                              // -r at the stage state
			const double sc = tc[s][2]*dt;
			S.each([&](size_t i, fvhip_ctx* h) {
				// the first stage has c1 = 0 and reads u in ustage's place; the last writes u
				launch_rk_stage(h->L.ncell, tc[s][0], tc[s][1], sc, h->M.area, h->d_r, us[i], s == 0 ? us[i] : ust[i],
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

}

using namespace fvhip_detail;

extern "C" {

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

}
