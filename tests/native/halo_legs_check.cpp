// Host shim of tests/test_halo_legs_host.py: partitions a mesh as fvhip_partition_graph does, builds every rank's
// Layout with the calls handle creation makes (extractPartition, buildLayout), then the leg table of
// halo_legs.hpp that fvhip_group_create stores, and hands the legs out. No device is touched.
#include "../../fvens_amd/csrc/halo_legs.hpp"
#include "../../fvens_amd/csrc/partition.hpp"

#include <exception>
#include <string>
#include <vector>

using namespace fvhip;

namespace {
std::string g_error;

struct Built {
	std::vector<Layout> L;
	HaloLegs legs;
};

HaloLegs legsOf(const std::vector<Layout>& Ls)
{
	std::vector<const Layout*> p;
	std::vector<int> rank;
	for(size_t i = 0; i < Ls.size(); i++) { p.push_back(&Ls[i]); rank.push_back(static_cast<int>(i)); }
	return haloLegs(p, rank);
}
}

extern "C" {

const char* hl_error() { return g_error.c_str(); }

void* hl_build(const fvhip_mesh* mesh, const fvhip_flow_config* cfg, int nparts, int layers)
{
	try {
		const std::vector<int> part = partitionGraph(*mesh, nparts);
		Built* B = new Built();
		for(int r = 0; r < nparts; r++) B->L.push_back(buildLayout(extractPartition(*mesh, part.data(), r, layers), *cfg, true));
		B->legs = legsOf(B->L);
		return B;
	} catch(const std::exception& e) {
		g_error = e.what();
		return nullptr;
	}
}

/// out[0..3]: neighbours, ghost rows, halo layers of the layout, legs of the rank
void hl_rank(void* h, int rank, int* out)
{
	const Built* B = static_cast<const Built*>(h);
	const Layout& L = B->L[rank];
	out[0] = static_cast<int>(L.nbr_rank.size()); out[1] = L.nghost; out[2] = L.halo_layers;
	out[3] = static_cast<int>(B->legs.of[rank].size());
}

/// per leg k of the rank, 8 ints: neighbour rank, peer, kk, ghost_start[k], this side's ghost counts of a one-
/// and a two-layer exchange, the peer's send counts of the same
void hl_legs(void* h, int rank, int* out)
{
	const Built* B = static_cast<const Built*>(h);
	const Layout& L = B->L[rank];
	for(size_t k = 0; k < B->legs.of[rank].size(); k++) {
		const HaloLeg& g = B->legs.of[rank][k];
		const int v[8] = {L.nbr_rank[k], g.peer, g.kk, L.ghost_start[k], ghostCount(L, k, 1), ghostCount(L, k, 2),
		                  sendCount(B->L[g.peer], g.kk, 1), sendCount(B->L[g.peer], g.kk, 2)};
		for(int j = 0; j < 8; j++) out[8*k + j] = v[j];
	}
}

/// the table of a damaged copy of the layouts: how 0 drops `rank`'s last neighbour from its nbr_rank, how 1
/// lengthens its last send block by one row. Returns what haloLegs throws ("" if it accepts the lists).
const char* hl_broken(void* h, int rank, int how)
{
	std::vector<Layout> Ls = static_cast<const Built*>(h)->L;
	if(how == 0) Ls[rank].nbr_rank.pop_back();
	else Ls[rank].send_start.back() += 1;
	try { legsOf(Ls); g_error.clear(); }
	catch(const std::exception& e) { g_error = e.what(); }
	return g_error.c_str();
}

void hl_free(void* h) { delete static_cast<Built*>(h); }

}
