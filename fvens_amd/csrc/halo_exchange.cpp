/** \file halo_exchange.cpp
 * \brief The halo transport: ghost rows of any array and face traces, between the RCCL ranks of a partition
 *   (one point-to-point group), inside a periodic handle (a gather on its device), or between the handles of a
 *   group held by one process (device copies along the legs fvhip_group_create built, halo_legs.hpp).
 */
#include "system.hpp"

void fvhip_ctx::pack(const double* arr, int width, hipStream_t st) {
	if(!st) st = stream;
	timed_on(st, "k_pack", [&]{ launch_pack_rows(d_send, nsend, arr, width, d_sendbuf, st); });
}

void fvhip_ctx::trace_pack(const double* left, int width, hipStream_t st) {
	if(L.trace_conn.empty()) throw std::logic_error("face-trace exchange: not a per-rank mesh (no connectivity faces)");
	if(width < 1 || width > 4) throw std::invalid_argument("face-trace exchange: width must be 1..4");
	timed_on(st, "k_pack", [&]{ launch_pack_rows(d_trace_conn, nsend, left, width, d_sendbuf, st); });
}

void fvhip_ctx::trace_unpack(double* right, int width, hipStream_t st) {
	timed_on(st, "k_unpack", [&]{ launch_unpack_rows(d_trace_conn, L.nghost, d_tracebuf, width, right, st); });
}

/// one RCCL point-to-point group with every neighbour rank on stream st: neighbour k's block of `send` (from row
/// send_start[k]) out, its block of `recv` (from row ghost_start[k]) in, `width` doubles per row, the leading
/// `layers` layers of each block. Both sides derive the counts from the same lists, so a leg with nothing to
/// move is skipped on both.
static void p2p(const fvhip_ctx* h, const double* send, double* recv, int width, int layers, hipStream_t st) {
	const Layout& L = h->L;
	NC(ncclGroupStart());
	for(size_t k = 0; k < L.nbr_rank.size(); k++) {
		const int q = L.nbr_rank[k];
		const size_t ns = static_cast<size_t>(sendCount(L, k, layers));
		const size_t ng = static_cast<size_t>(ghostCount(L, k, layers));
		if(ns) NC(ncclSend(send + static_cast<size_t>(width)*L.send_start[k], width*ns, ncclDouble, q, h->comm, st));
		if(ng) NC(ncclRecv(recv + static_cast<size_t>(width)*L.ghost_start[k], width*ng, ncclDouble, q, h->comm, st));
	}
	NC(ncclGroupEnd());
}

void fvhip_ctx::trace_exchange_rccl(const double* left, double* right, int width) {
	if(periodic) {        // right[ic] = left[partner(ic)] in one launch
		if(width < 1 || width > 4) throw std::invalid_argument("face-trace exchange: width must be 1..4");
		if(left == right) throw std::invalid_argument("face-trace exchange: left and right must be different arrays");
		timed("k_ghost_gather", [&]{ launch_ghost_gather(d_trace_from, L.nghost, left, width, right, 0, stream); });
		HC(hipGetLastError());
		return;
	}
	if(!comm) throw std::runtime_error("face-trace exchange: call fvhip_comm_init (or use a group) first");
	trace_pack(left, width, stream);
	p2p(this, d_sendbuf, d_tracebuf, width, 2, stream);      // whole blocks: a trace list has no layers
	trace_unpack(right, width, stream);
}

void fvhip_ctx::exchange_rccl(double* arr, int width, hipStream_t st, int layers) {
	if(!halo()) return;
	if(!st) st = stream;
	if(periodic) {        // ghost row g = the row of the partner cell d_send[g]: one launch, no buffer
		if(width < 1 || width > 8) throw std::invalid_argument("ghost exchange: width must be 1..8");
		timed_on(st, "k_ghost_gather", [&]{ launch_ghost_gather(d_send, L.nghost, arr, width, arr, L.ncell, st); });
		HC(hipGetLastError());
		return;
	}
	if(!comm) throw std::runtime_error("partitioned handle: call fvhip_comm_init (or use a group) first");
	pack(arr, width, st);
	p2p(this, d_sendbuf, arr + static_cast<size_t>(width)*L.ncell, width, layers, st);
}

namespace fvhip_detail {

void System::copyLegs(size_t i, double* dst, int width, int layers, hipStream_t st, bool after_pack) const {
	const Layout& L = hs[i]->L;
	for(size_t k = 0; k < legs->of[i].size(); k++) {
		const HaloLeg& leg = legs->of[i][k];
		const fvhip_ctx* q = hs[leg.peer];
		const int cnt = ghostCount(L, k, layers);      // = the peer's send count (haloLegs)
		if(cnt == 0) continue;
		if(after_pack) HC(hipStreamWaitEvent(st, q->ev_packed, 0));
		HC(hipMemcpyAsync(dst + static_cast<size_t>(width)*L.ghost_start[k],
		                  q->d_sendbuf + static_cast<size_t>(width)*q->L.send_start[leg.kk],
		                  sizeof(double)*width*static_cast<size_t>(cnt), hipMemcpyDeviceToDevice, st));
	}
}

void System::exchange(const ArrayOf& arr, int width, int layers) {
	if(!legs) {
		if(halo()) each([&](size_t i, fvhip_ctx* h) { h->exchange_rccl(arr(i), width, nullptr, layers); });
		return;
	}
	if(!legs->any) return;
	// in-process exchange: pack everywhere, then copy each neighbour's packed rows into the ghost block
	const size_t n = hs.size();
	for(size_t i = 0; i < n; i++) if(hs[i]->halo()) { HC(hipSetDevice(hs[i]->device)); hs[i]->pack(arr(i), width); }
	for(size_t i = 0; i < n; i++) HC(hipStreamSynchronize(hs[i]->stream));
	for(size_t i = 0; i < n; i++) copyLegs(i, arr(i) + static_cast<size_t>(width)*hs[i]->L.ncell, width, layers, hs[i]->stream);
	for(size_t i = 0; i < n; i++) HC(hipStreamSynchronize(hs[i]->stream));
}

void System::traceExchange(const double* const* left, double* const* right, int width) {
	each([&](size_t i, fvhip_ctx* h) { h->trace_pack(left[i], width, h->stream); });
	for(fvhip_ctx* h : hs) HC(hipStreamSynchronize(h->stream));
	each([&](size_t i, fvhip_ctx* h) {
		copyLegs(i, h->d_tracebuf, width, 2, h->stream);      // whole blocks
		h->trace_unpack(right[i], width, h->stream);
	});
	for(fvhip_ctx* h : hs) HC(hipStreamSynchronize(h->stream));
}

}
