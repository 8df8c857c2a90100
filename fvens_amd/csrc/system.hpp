/** \file system.hpp
 * \brief One global system: a handle, or all ranks of a partition driven from one process (a group), with its
 *   halo transport (halo_exchange.cpp) and the residual over it (residual.cpp). The implicit solver's operator
 *   and preconditioner on a system are in linop.hpp.
 */
#ifndef FVHIP_SYSTEM_HPP
#define FVHIP_SYSTEM_HPP

#include "ctx.hpp"
#include "halo_legs.hpp"

#include <functional>
#include <vector>

/// all ranks of one partition driven from one process (fvhip_group_*); the legs are built by fvhip_group_create
struct fvhip_group_s { std::vector<fvhip_ctx*> hs; fvhip::HaloLegs legs; };

namespace fvhip_detail {

typedef std::function<double*(size_t)> ArrayOf;

struct System
{
	std::vector<fvhip_ctx*> hs;
	/// a group's in-process transport (device copies along these legs); null: one handle, which exchanges
	/// with RCCL, or on its own device if periodic
	const HaloLegs* legs = nullptr;

	size_t size() const { return hs.size(); }
	bool halo() const { return hs[0]->halo(); }
	template <typename F> void each(F&& f) {
		for(size_t i = 0; i < hs.size(); i++) { HC(hipSetDevice(hs[i]->device)); f(i, hs[i]); }
	}
	/// fills the ghost rows of every handle's array (`width` doubles per row): both layers of a two-layer
	/// halo with layers 2 (the residual's state), else the first (gradients, limiter values, Krylov vectors)
	void exchange(const ArrayOf& arr, int width, int layers = 1);
	/// handle i's ghost blocks, `width` doubles per row, copied from its peers' send buffers to `dst` on `st`
	/// (groups); after_pack: each copy waits for the sender's ev_packed
	void copyLegs(size_t i, double* dst, int width, int layers, hipStream_t st, bool after_pack = false) const;
	/// L2TraceVector::updateSharedFacesBegin/End over a group: fvhip_ctx::traceExchange with device copies
	void traceExchange(const double* const* left, double* const* right, int width);
	/// the steppers' residual: every handle's d_r = 0 + (-r(us)) with its local time steps in d_dtm; fills the
	/// ghost rows of us
	void residual(const std::vector<double*>& us);
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
	/// the global minimum of every handle's local time steps d_dtm, on the host (the explicit drivers' dtmin):
	/// per handle launch_min over its owned cells, ncclMin over its ranks and the copy, then the waits and the
	/// minimum over the handles. -inf if a time step is NaN (launch_min), so the caller's finiteness check fires
	double allmin() {
		each([&](size_t, fvhip_ctx* h) {
			launch_min(h->L.ncell, h->d_dtm, h->iw.part, h->iw.red, h->stream);
			if(h->comm) NC(ncclAllReduce(h->iw.red, h->iw.red, 1, ncclDouble, ncclMin, h->comm, h->stream));
			HC(hipMemcpyAsync(h->iw.h_red, h->iw.red, sizeof(double), hipMemcpyDeviceToHost, h->stream));
		});
		double m = INFINITY;
		each([&](size_t, fvhip_ctx* h) { HC(hipStreamSynchronize(h->stream)); m = std::min(m, h->iw.h_red[0]); });
		return m;
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

inline System single(fvhip_ctx* h)
{
	if(h->in_group) throw std::runtime_error("handle belongs to a group: use the fvhip_group_* entry point");
	if(h->needsComm()) throw std::runtime_error("partitioned handle: call fvhip_comm_init (or use a group) first");
	return System{{h}};
}

inline System ofGroup(fvhip_group_s* g) { return System{g->hs, &g->legs}; }

/// The device sweep over a system: -r(us[i]) added (or written) into rs[i], time steps into dts[i] (null
/// entries: none). On a partitioned mesh us[i] has room for the ghost rows (ncell+nghost rows), which this fills
/// (ResidualPath::HaloReady: which the caller has filled). One array entry per handle. residual.cpp
void residual(System& S, const double* const* us, double* const* rs, bool dt, double* const* dts, bool overwrite,
              ResidualPath path = ResidualPath::Default);

inline void System::residual(const std::vector<double*>& us) {
	std::vector<double*> rs, dts;
	for(fvhip_ctx* h : hs) { rs.push_back(h->d_r); dts.push_back(h->d_dtm); }
	fvhip_detail::residual(*this, us.data(), rs.data(), true, dts.data(), true);
}

/// MatrixFreeSpatialJacobian::apply (alinalg.cpp:142-233) over a system (implicit.cpp): |x| is the global norm
/// (launch_mdot + launch_pertmag on the solver's reduction scratch). fvhip_ctx::matfree is the single-domain
/// operator of the standalone entry points, with launch_mf_norm on scratch of its own: the two may differ in
/// the last bits of |x| and stay apart.
/// have_norm: |x|^2 is already in iw.red (the line solve that produced x summed it, LinOp::precondition)
void matfreeApply(System& S, const ArrayOf& x, const ArrayOf& y, bool have_norm = false);

typedef std::vector<double*> States;

/// a stepper's entry point on one handle / on a group (implicit.cpp, explicit.cpp): the arguments checked (have:
/// its other pointers are there), the system made, `step(S, states)` run and waited for
template <typename F> int onHandle(fvhip_handle h, double* d_u, bool have, F&& step)
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
template <typename F> int onGroup(fvhip_group g, double* const* d_u, bool have, F&& step)
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
#endif
