// Host shim of tests/test_ilu_order_host.py: builds a Layout with the calls handle creation makes (as
// precond_host_check.cpp does), runs precond_setup.cpp's iluOrder on its cell graph and hands out the rank, the
// depth and the owned cells' interior faces. No device is touched.
#include "../../fvens_amd/csrc/precond_setup.hpp"
#include "../../fvens_amd/csrc/layout.hpp"
#include "../../fvens_amd/csrc/partition.hpp"

#include <algorithm>
#include <exception>
#include <string>
#include <vector>

using namespace fvhip;

namespace {
std::string g_error;

struct Built {
	std::vector<std::vector<int>> arrays;      // 0: {ncell, nghost, depth}, 1: rank, 2: if_L, 3: if_R
};
}

extern "C" {

const char* io_error() { return g_error.c_str(); }

void* io_build(const fvhip_mesh* mesh, const fvhip_flow_config* cfg, int nparts, int rank, int order)
{
	try {
		Layout L;
		if(nparts > 1) {
			const std::vector<int> part = partitionRCB(mesh->rc, mesh->nelem, nparts);
			L = buildLayout(extractPartition(*mesh, part.data(), rank, 2), *cfg, true);
		} else L = buildLayout(topoFromMesh(*mesh), *cfg, true);
		const IluOrder O = iluOrder(cellGraph(L), order);
		Built* B = new Built();
		B->arrays.resize(4);
		B->arrays[0] = {L.ncell, L.nghost, O.depth};
		B->arrays[1] = O.rank;
		B->arrays[2] = L.if_L; B->arrays[3] = L.if_R;
		return B;
	} catch(const std::exception& e) {
		g_error = e.what();
		return nullptr;
	}
}

long long io_size(void* h, int what)
{
	const Built* B = static_cast<const Built*>(h);
	return what >= 0 && what < static_cast<int>(B->arrays.size()) ? static_cast<long long>(B->arrays[what].size()) : 0;
}

void io_copy(void* h, int what, int* out)
{
	const std::vector<int>& a = static_cast<const Built*>(h)->arrays[static_cast<size_t>(what)];
	std::copy(a.begin(), a.end(), out);
}

void io_free(void* h) { delete static_cast<Built*>(h); }

}
