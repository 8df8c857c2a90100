/** \file residual.cpp
 * \brief The residual over a system (system.hpp): the stage launchers of one handle and the schedules that
 *   order them -- fused in one launch, fused and overlapped with the halo exchange, staged, pipelined.
 */
#include "system.hpp"

void fvhip_ctx::stage_gradients(const double* u) {
	if(L.nghost > 0)
		timed("k_ghost_prim", [&]{ launch_cons2prim_rows(P.gas, u, d_up, L.ncell, L.nghost, stream); });
	if(cfg.gradientscheme == FVHIP_GRAD_LEASTSQUARES) {
		// limited reconstructions: the limiter values come out of the same kernel
		timed("k_prep_grad_wls", [&]{ KOPS(launch_prep_grad_wls)(M, P, u, d_up, d_ubc, d_ug, d_grad, stream, 0, -1,
		                                                         limKind(), d_phi); });
	} else {
		timed("k_prep", [&]{ KOPS(launch_prep)(M, P, u, d_up, d_ubc, d_ug, true, stream); });
		if(cfg.gradientscheme == FVHIP_GRAD_GREENGAUSS)
			timed("k_grad_gg", [&]{ KOPS(launch_grad_gg)(M, d_up, d_ug, d_grad, stream); });
		else KOPS(launch_fill)(d_grad, 0.0, 8LL*ntotal(), stream);
	}
}

void fvhip_ctx::stage_limiter() {
	if(fusedLimiter()) return;
	const int venk = cfg.reconstruction == FVHIP_REC_VENKATAKRISHNAN;
	timed("k_limiter", [&]{ KOPS(launch_limiter)(M, P, venk, d_up, d_ug, d_grad, d_phi, stream); });
}

void fvhip_ctx::stage_weno() { timed("k_weno", [&]{ KOPS(launch_weno)(M, P, d_grad, d_lgrad, stream); }); }

/// the head every sweep launch's buffers share
static SweepBuffers sweepHead(const double* u, double* r, double* dtm, bool overwrite, const int* plist, int pcount) {
	SweepBuffers B{};
	B.u = u; B.r = r; B.dtm = dtm; B.overwrite = overwrite ? 1 : 0;
	B.plist = plist; B.pcount = pcount;
	return B;
}

void fvhip_ctx::stage_sweep(const double* u, double* r, bool dt, double* dtm, bool overwrite,
                            const int* plist, int pcount, hipStream_t st) {
	if(!st) st = stream;
	const int rk = recKind();
	SweepBuffers B = sweepHead(u, r, dtm, overwrite, plist, pcount);
	if(rk != SR_FIRST) {
		B.up = d_up; B.grad = d_grad; B.rgrad = d_grad; B.ubc = d_ubc; B.ug = d_ug;
		if(limited()) B.phi = d_phi;
		if(cfg.reconstruction == FVHIP_REC_WENO) B.rgrad = d_lgrad;
	}
	const char* nm = nullptr;
	// name is only known after launch; record under a generic label then rename
	timed_on(st, "k_sweep", [&]{ nm = KOPS(launch_sweep)(M, P, B, cfg.conv_numflux, rk, viscKind(), dt, st); });
	if(prof && !recs.empty() && recs.back().name == "k_sweep" && nm) recs.back().name = nm;
	HC(hipGetLastError());
}

void fvhip_ctx::stage_border_gradients(const double* u, hipStream_t st) {
	if(!st) st = stream;
	timed_on(st, "k_grad_wls_list", [&]{ KOPS(launch_grad_wls_list)(M, P, u, d_border, nborder, d_grad, st); });
}

void fvhip_ctx::stage_ghost_gradients(const double* u, hipStream_t st) {
	if(!st) st = stream;
	timed_on(st, "k_grad_ghost", [&]{ KOPS(launch_grad_ghost)(M, P, u, d_grad, st, limKind(), d_phi); });
}

void fvhip_ctx::stage_fused(const double* u, double* r, bool dt, double* dtm, bool overwrite,
                            const int* plist, int pcount, hipStream_t st, const MfFuse& mf) {
	if(!st) st = stream;
	if(plist && pcount == 0) return;
	SweepBuffers B = sweepHead(u, r, dtm, overwrite, plist, pcount);
	B.grad = d_grad;     // received gradients of ghost cells (partitioned meshes)
	if(limited()) B.phi = d_phi;   // layer-1 ghosts' limiter values (two-layer halo)
	B.mfx = mf.x; B.mfpm = mf.pm; B.mfres = mf.res; B.mfmdt = mf.mdt;
#ifdef FVHIP_FZ_STAMPS
	{   // one buffer for the largest launch (all patches), zeroed so that blocks without a patch read 0
		const size_t words = 8*static_cast<size_t>(8*((M.npatch + 7)/8));
		if(!d_stamps) {
			void* p = nullptr;
			HC(hipMalloc(&p, words*sizeof(unsigned long long)));
			owned.push_back(p);
			d_stamps = static_cast<unsigned long long*>(p);
		}
		HC(hipMemsetAsync(d_stamps, 0, words*sizeof(unsigned long long), st));
		B.stamps = d_stamps;
		stamp_blocks = 8*(((plist ? pcount : M.npatch) + 7)/8);
	}
#endif
	const char* nm = nullptr;
	timed_on(st, "k_residual_wls", [&]{ nm = KOPS(launch_residual_wls)(M, P, B, cfg.conv_numflux, recKind(), viscKind(),
	                                                                       limKind(), dt, st); });
	if(prof && !recs.empty() && recs.back().name == "k_residual_wls" && nm) recs.back().name = nm;
	HC(hipGetLastError());
}

/// gradient chunks on `stream`; each sweep group on stream2 waits for the last chunk it reads.
/// Same kernels and arithmetic as the staged path, so bitwise its result.
void fvhip_ctx::residual_pipelined(const double* u, double* r, bool dt, double* dtm, bool overwrite) {
	const int K = static_cast<int>(L.pipe_cell_start.size()) - 1;
	if(!stream2) {
		HC(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
		pipe_ev.resize(K);
		for(hipEvent_t& e : pipe_ev) HC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		HC(hipEventCreateWithFlags(&pipe_start, hipEventDisableTiming));
		HC(hipEventCreateWithFlags(&pipe_done, hipEventDisableTiming));
	}
	HC(hipEventRecord(pipe_start, stream));          // everything the caller queued before
	HC(hipStreamWaitEvent(stream2, pipe_start, 0));
	for(int k = 0; k < K; k++) {
		timed("k_prep_grad_wls", [&]{
			KOPS(launch_prep_grad_wls)(M, P, u, d_up, d_ubc, d_ug, d_grad, stream, L.pipe_cell_start[k], L.pipe_cell_start[k+1], 0, nullptr);
		});
		HC(hipEventRecord(pipe_ev[k], stream));
	}
	for(int k = 0; k < K; k++) {
		const int n = L.pipe_group_start[k+1] - L.pipe_group_start[k];
		if(n == 0) continue;
		HC(hipStreamWaitEvent(stream2, pipe_ev[k], 0));
		stage_sweep(u, r, dt, dtm, overwrite, d_pipe_patch + L.pipe_group_start[k], n, stream2);
	}
	HC(hipEventRecord(pipe_done, stream2));
	HC(hipStreamWaitEvent(stream, pipe_done, 0));   // the residual completes on `stream`
}

/// staged wins over pipelined; FVHIP_RES_HALO_READY is refused where no fused single-exchange residual exists
ResidualPath fvhip_ctx::residualPath(int flags) const {
	const ResidualPath p = (flags & FVHIP_RES_STAGED) ? ResidualPath::Staged
	                     : (flags & FVHIP_RES_PIPELINED) ? ResidualPath::Pipelined : ResidualPath::Default;
	if(!(flags & FVHIP_RES_HALO_READY) || !halo()) return p;       // without ghost rows there is nothing to be ready
	if(!fused(p) || !singleExchange())
		throw std::runtime_error("FVHIP_RES_HALO_READY: only the fused single-exchange configurations (two-layer "
		                         "halo, WLS + MUSCL / linear / Barth-Jespersen / Venkatakrishnan)");
	return ResidualPath::HaloReady;
}

void fvhip_ctx::residual(const double* u, double* r, bool dt, double* dtm, bool overwrite, ResidualPath path) {
	System S{{this}};
	fvhip_detail::residual(S, &u, &r, dt, &dtm, overwrite, path);
}

namespace fvhip_detail {

/// the second stream and events of the overlapped fused residual
static void ensureOverlap(fvhip_ctx* h) {
	if(h->comm_stream) return;
	HC(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
	for(hipEvent_t* e : {&h->ev_u, &h->ev_halo, &h->ev_packed, &h->ev_copied}) HC(hipEventCreateWithFlags(e, hipEventDisableTiming));
}

/// The fused residual overlapped with the halo exchange, of one RCCL (or periodic) handle or of a group: the
/// halo -- ghost u, ghost (or border, exchanged) gradients -- arrives on each handle's comm_stream while the
/// interior patches run on its `stream`; the border patches are launched on comm_stream right behind the halo, so
/// their blocks fill the interior launch's last partial wave instead of forming a fraction-of-a-wave launch after
/// it. The two launches write disjoint cells; `stream` joins the comm stream before the residual is complete.
/// The kinds of system differ in the transport alone. RCCL sends and receives in one call, enqueued before the
/// interior patches. A group (single-exchange configurations) packs before them and copies behind them, each copy
/// waiting on the sender's pack, and a send buffer is refilled only after every receiver has copied the previous
/// exchange out of it (ev_packed, ev_copied): the stream/event ordering and the send-buffer reuse of the RCCL
/// path therefore run (and are checked bitwise against one GPU) with several ranks on one device, where RCCL
/// cannot. (No hipGraph capture of the RCCL step: DESIGN.md section 6.)
static void residualOverlapped(System& S, const double* const* us, double* const* rs, bool dt, double* const* dts,
                               bool overwrite) {
	const size_t n = S.size();
	const bool group = S.legs != nullptr;
	// every stage launches on the handle's own device (a group may span devices)
	auto on = [&](size_t i) -> fvhip_ctx* { if(group) HC(hipSetDevice(S.hs[i]->device)); return S.hs[i]; };
	// 1. the comm stream takes u as the caller left it (and r, dtm free) and sends
	for(size_t i = 0; i < n; i++) {
		fvhip_ctx* h = on(i);
		double* u = const_cast<double*>(us[i]);
		ensureOverlap(h);
		HC(hipEventRecord(h->ev_u, h->stream));
		HC(hipStreamWaitEvent(h->comm_stream, h->ev_u, 0));
		if(group) {
			for(fvhip_ctx* q : S.hs) if(q->copied_recorded) HC(hipStreamWaitEvent(h->comm_stream, q->ev_copied, 0));
			h->pack(u, 4, h->comm_stream);
			HC(hipEventRecord(h->ev_packed, h->comm_stream));
		} else if(h->singleExchange()) {
			h->exchange_rccl(u, 4, h->comm_stream, 2);
			h->stage_ghost_gradients(u, h->comm_stream);
		} else {
			h->exchange_rccl(u, 4, h->comm_stream);
			h->stage_border_gradients(u, h->comm_stream);
			h->exchange_rccl(h->d_grad, 8, h->comm_stream);
		}
	}
	// 2. the patches that read no halo data
	for(size_t i = 0; i < n; i++)
		on(i)->stage_fused(us[i], rs[i], dt, dts[i], overwrite, S.hs[i]->d_fz_order, S.hs[i]->L.fz_ninner);
	for(size_t i = 0; i < n; i++) {
		fvhip_ctx* h = on(i);
		if(group) {   // 3. receive both halo layers, then the layer-1 ghost gradients
			S.copyLegs(i, const_cast<double*>(us[i]) + 4*static_cast<size_t>(h->L.ncell), 4, 2, h->comm_stream, true);
			h->stage_ghost_gradients(us[i], h->comm_stream);
			HC(hipEventRecord(h->ev_copied, h->comm_stream));
		}
		// 4. the border patches on the comm stream right behind the halo
		h->stage_fused(us[i], rs[i], dt, dts[i], overwrite, h->d_fz_order + h->L.fz_ninner,
		               static_cast<int>(h->L.fz_order.size()) - h->L.fz_ninner, h->comm_stream);
		HC(hipEventRecord(h->ev_halo, h->comm_stream));
	}
	if(group) for(fvhip_ctx* h : S.hs) h->copied_recorded = true;
	// 5. the residual completes on each handle's stream; later work there (the next pack of a
	//    synchronous exchange included) also follows every copy out of its send buffer
	for(size_t i = 0; i < n; i++) {
		fvhip_ctx* h = on(i);
		HC(hipStreamWaitEvent(h->stream, h->ev_halo, 0));
		if(group) for(fvhip_ctx* q : S.hs) HC(hipStreamWaitEvent(h->stream, q->ev_copied, 0));
	}
}

void residual(System& S, const double* const* us, double* const* rs, bool dt, double* const* dts, bool overwrite,
              ResidualPath path) {
	std::vector<fvhip_ctx*>& hs = S.hs;
	fvhip_ctx* h0 = hs[0];
	const bool single = h0->singleExchange();
	// every stage launches on the handle's own device (a group may span devices)
	auto on = [&](size_t i) -> fvhip_ctx* { HC(hipSetDevice(hs[i]->device)); return hs[i]; };
	auto state = [&](size_t i) { return const_cast<double*>(us[i]); };
	if(path == ResidualPath::HaloReady) {
		// the ghost rows of u are current (residualPath has checked the configuration): layer-1 ghost gradients
		// (and limiter values), then every patch on the handle's stream
		for(size_t i = 0; i < hs.size(); i++) {
			on(i)->stage_ghost_gradients(us[i]);
			hs[i]->stage_fused(us[i], rs[i], dt, dts[i], overwrite, hs[i]->d_fz_order, static_cast<int>(hs[i]->L.fz_order.size()));
		}
		return;
	}
	if(hs.size() == 1 && !S.legs && h0->pipelined(path)) {
		h0->residual_pipelined(us[0], rs[0], dt, dts[0], overwrite);
		return;
	}
	if(h0->fused(path)) {
		if(h0->halo()) {
			if((hs.size() == 1 && !S.legs) || (single && S.legs)) { residualOverlapped(S, us, rs, dt, dts, overwrite); return; }
			// interior patches need no halo data: they run first, then the exchange of the ghost
			// rows of u and of the gradients of the cells other ranks hold as ghosts, then the rest
			for(size_t i = 0; i < hs.size(); i++)
				on(i)->stage_fused(us[i], rs[i], dt, dts[i], overwrite, hs[i]->d_fz_order, hs[i]->L.fz_ninner);
			if(single) {
				S.exchange(state, 4, 2);
				for(size_t i = 0; i < hs.size(); i++) on(i)->stage_ghost_gradients(us[i]);
			} else {
				S.exchange(state, 4);
				for(size_t i = 0; i < hs.size(); i++) on(i)->stage_border_gradients(us[i]);
				S.exchange([&](size_t i) { return hs[i]->d_grad; }, 8);
			}
			for(size_t i = 0; i < hs.size(); i++)
				on(i)->stage_fused(us[i], rs[i], dt, dts[i], overwrite, hs[i]->d_fz_order + hs[i]->L.fz_ninner,
				                   static_cast<int>(hs[i]->L.fz_order.size()) - hs[i]->L.fz_ninner);
			return;
		}
		for(size_t i = 0; i < hs.size(); i++) on(i)->stage_fused(us[i], rs[i], dt, dts[i], overwrite);
		return;
	}
	S.exchange(state, 4, h0->L.halo_layers);
	if(h0->recKind() != SR_FIRST) {
		for(size_t i = 0; i < hs.size(); i++) on(i)->stage_gradients(us[i]);
		if(single) { for(size_t i = 0; i < hs.size(); i++) on(i)->stage_ghost_gradients(us[i]); }
		else S.exchange([&](size_t i) { return hs[i]->d_grad; }, 8);
		if(h0->limited() && !single) {      // single exchange: the ghosts' limiter values are local
			for(size_t i = 0; i < hs.size(); i++) on(i)->stage_limiter();
			S.exchange([&](size_t i) { return hs[i]->d_phi; }, 4);
		}
		if(h0->cfg.reconstruction == FVHIP_REC_WENO) {
			for(size_t i = 0; i < hs.size(); i++) on(i)->stage_weno();
			S.exchange([&](size_t i) { return hs[i]->d_lgrad; }, 8);
		}
	}
	for(size_t i = 0; i < hs.size(); i++) on(i)->stage_sweep(us[i], rs[i], dt, dts[i], overwrite);
}

}
