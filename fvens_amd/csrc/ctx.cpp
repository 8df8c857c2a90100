/** \file ctx.cpp
 * \brief What a handle allocates or builds on first use -- Jacobian mesh view, work space of the drivers, the
 *   surface cache, transfer scratch -- and the single-domain matrix-free operator.
 */
#include "ctx.hpp"

double* fvhip_ctx::rawScratch(size_t doubles) {
	if(raw_cap < doubles) {
		if(d_raw) { HC(hipStreamSynchronize(stream)); release(d_raw); }   // no transfer still reading it
		d_raw = dalloc(doubles, owned);
		raw_cap = doubles;
	}
	return d_raw;
}

void fvhip_ctx::release(const void* p) {
	if(!p) return;
	auto it = std::find(owned.begin(), owned.end(), p);
	if(it == owned.end()) throw std::logic_error("release: not a buffer of this handle");
	(void)hipFree(*it);
	owned.erase(it);
}

void fvhip_ctx::ensureJacobian() {
	const int jf = cfg.conv_numflux_jac;
	if(jf == FVHIP_FLUX_VANLEER) throw std::runtime_error(" ! VanLeerFlux: Not implemented!");   // anumericalflux.cpp:253-257
	if(jf == FVHIP_FLUX_AUSMPLUS) throw std::runtime_error(" ! AUSMPlusFlux: Not implemented!"); // :556-560
	if(jf < 0 || jf > 6) throw std::invalid_argument("unknown Jacobian flux");
	for(int i = 0; i < cfg.nbc; i++)
		if(bc_type[i] == FVHIP_BC_SUBSONIC_INFLOW)   // InFlow::computeGhostStateAndJacobian, abc.cpp:178-185
			throw std::runtime_error("subsonic inflow BC has no Jacobian (Not implemented!)");
	if(jac_ready) return;
	auto& o = owned;
	J.ncell = L.ncell; J.nbface = L.nbface; J.ninface = L.ninface;
	J.if_LR = reinterpret_cast<const int2*>(upload(pack2(L.if_L, L.if_R), o));
	J.if_n = reinterpret_cast<const double2*>(upload(L.if_n, o));
	J.if_len = upload(L.if_len, o);
	J.bf_L = M.bf_L; J.bf_bc = M.bf_bc; J.bf_n = M.bf_n; J.bf_rcbp = M.bf_rcbp; J.rc = M.rc;
	J.bf_len = upload(L.bf_len, o);
	J.cell_rfaces = reinterpret_cast<const int4*>(upload(L.cell_rfaces, o));
	J.cell_nbr_fo = M.cell_nbr_fo;
	d_jb = dalloc(16*static_cast<size_t>(std::max(L.nbface,1)), o);
	jac_ready = true;
}

void fvhip_ctx::assemble(const double* u, double* diag, double* lower, double* upper, double cfl, double* dtm) {
	ensureJacobian();
	timed("k_jac_faces", [&]{ launch_jac_faces(J, P, cfg.conv_numflux_jac, viscKind(), u, d_jb, lower, upper, stream); });
	timed("k_jac_diag", [&]{ launch_jac_diag(J, d_jb, lower, upper, diag, stream, cfl > 0 ? M.area : nullptr, cfl, dtm); });
	HC(hipGetLastError());
}

void fvhip_ctx::ensureReductions() {
	if(iw.red) return;
	auto& o = owned;
	iw.red = dalloc(KRY_MAXK + 2, o); iw.coef = dalloc(KRY_MAXK + 2, o); iw.pm = dalloc(2, o);
	iw.part = dalloc(kry_scratch(2), o);
	for(double** hp : {&iw.h_red, &iw.h_coef, &iw.h_red2}) {
		void* p = nullptr;
		HC(hipHostMalloc(&p, (KRY_MAXK + 2)*sizeof(double), hipHostMallocDefault));
		owned_host.push_back(p);
		*hp = static_cast<double*>(p);
	}
}

void fvhip_ctx::ensureVectors() {
	ensureReductions();
	if(iw.z) return;
	const size_t N = static_cast<size_t>(L.ncell), NT = N + static_cast<size_t>(L.nghost);
	auto& o = owned;
	iw.z = dalloc(4*NT, o); iw.aux = dalloc(4*NT, o);
	iw.w = dalloc(4*N, o); iw.t = dalloc(4*N, o); iw.s = dalloc(4*N, o); iw.du = dalloc(4*N, o);
	iw.yg = dalloc(4*N, o);
}

void fvhip_ctx::ensureImplicit(int m) {
	ensureJacobian();
	ensureVectors();
	const size_t N = static_cast<size_t>(L.ncell);
	const size_t Fi = static_cast<size_t>(std::max(L.ninface, 1));
	auto& o = owned;
	if(!iw.jd) {
		iw.jd = dalloc(16*N, o); iw.jlo = dalloc(16*Fi, o); iw.jup = dalloc(16*Fi, o); iw.dinv = dalloc(16*N, o);
	}
	if(iw.m < m) {                  // a larger basis: the old one stays owned until destroy
		iw.V = dalloc(4*N*static_cast<size_t>(m + 1), o);
		iw.part = dalloc(kry_scratch(m + 2), o);
		iw.m = m;
	}
}

fvhip_ctx::SurfCache& fvhip_ctx::surfaceFaces(int marker) {
	auto it = surf.find(marker);
	if(it != surf.end()) return it->second;
	std::vector<int> Lc;
	std::vector<double> geo;
	for(int f = 0; f < L.nbface; f++) {
		if(L.bf_tag[f] != marker) continue;
		Lc.push_back(L.bf_L[f]);
		const double g5[5] = {L.bf_n[2*f], L.bf_n[2*f+1], L.bf_len[f], L.bf_gr[2*f], L.bf_gr[2*f+1]};
		geo.insert(geo.end(), g5, g5 + 5);
	}
	SurfCache c;
	c.S.n = static_cast<int>(Lc.size());
	if(c.S.n > 0) {
		c.S.L = upload(Lc, owned);
		c.S.geo = upload(geo, owned);
		c.faceout = dalloc(4*Lc.size(), owned);
		c.contrib = dalloc(4*Lc.size(), owned);
	}
	c.sums = dalloc(4, owned);
	return surf.emplace(marker, c).first->second;
}

void fvhip_ctx::matfree(const double* x, double* y) {
	if(!mf_u || !mf_r || !mf_mdt) throw std::runtime_error("matrix-free operator: state not set");
	if(halo()) throw std::logic_error("fvhip_ctx::matfree is the single-domain operator (partitioned: sysMatfree)");
	const size_t N = static_cast<size_t>(L.ncell);
	if(!d_part) { d_part = dalloc(mf_partials(), owned); d_pm = dalloc(2, owned); }
	if(!d_mf_aux) { d_mf_aux = dalloc(4*N, owned); d_mf_y = dalloc(4*N, owned); }
	timed("k_mf_norm", [&]{ launch_mf_norm(4LL*L.ncell, x, mf_eps, d_part, d_pm, stream); });
	if(matfreeFusable() && matfreeNoAlias(mf_u, x, y)) {
		stage_fused(mf_u, y, false, nullptr, true, nullptr, 0, nullptr, MfFuse{x, d_pm, mf_r, mf_mdt});
		return;
	}
	timed("k_mf_perturb", [&]{ launch_mf_perturb(4LL*L.ncell, mf_u, x, d_pm, d_mf_aux, stream); });
	residual(d_mf_aux, d_mf_y, false, nullptr, true);
	timed("k_mf_combine", [&]{ launch_mf_combine(L.ncell, mf_mdt, x, d_mf_y, mf_r, d_pm, y, stream); });
	HC(hipGetLastError());
}
