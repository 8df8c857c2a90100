// Host shim of tests/test_amg_blocks_host.py: builds a Layout as handle creation does (buildLayout of
// topoFromMesh), runs the coarsening loop of fvhip_ctx::ensureAmg on it and hands out every level's colour order
// and, for a given number of rows per block, the block smoother's (block, colour) offsets (amg.cpp
// amgBlockOffsets) -- what fvhip_ctx::amgBlocks uploads. No device is touched.
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
	std::vector<AmgLevelHost> levels;
	std::vector<int> out;                    // the array asked for last (ab_get)
};
}

extern "C" {

const char* ab_error() { return g_error.c_str(); }

void* ab_build(const fvhip_mesh* mesh, const fvhip_flow_config* cfg, int amg_levels, double amg_thr)
{
	try {
		const Layout L = buildLayout(topoFromMesh(*mesh), *cfg, true);
		Built* B = new Built();
		AmgGraph g = amgFineGraph(cellGraph(L));
		for(int l = 1; l < amg_levels; l++) {            // fvhip_ctx::ensureAmg's loop and stop rules
			if(g.n < 64) break;
			AmgLevelHost H = amgCoarsen(g, amg_thr);
			if(H.n*5 > g.n*4) break;
			g = amgGraphOf(H);
			B->levels.push_back(std::move(H));
		}
		return B;
	} catch(const std::exception& e) {
		g_error = e.what();
		return nullptr;
	}
}

int ab_levels(void* h) { return static_cast<int>(static_cast<const Built*>(h)->levels.size()); }

/// what = 0: rows (one value), 1: the colour starts, 2: the rows colour by colour, 3: the offsets for blocks of
/// R rows; returns the length (-1: an error, see ab_error), the values stay until the next call (ab_copy)
long long ab_get(void* h, int level, int what, int R)
{
	try {
		Built* B = static_cast<Built*>(h);
		const AmgLevelHost& L = B->levels.at(static_cast<size_t>(level));
		if(what == 0) B->out = {L.n};
		else if(what == 1) B->out = L.cstart_colour;
		else if(what == 2) B->out = L.cells;
		else B->out = amgBlockOffsets(L.n, L.cstart_colour, L.cells, R);
		return static_cast<long long>(B->out.size());
	} catch(const std::exception& e) {
		g_error = e.what();
		return -1;
	}
}

void ab_copy(void* h, int* out)
{
	const std::vector<int>& a = static_cast<const Built*>(h)->out;
	std::copy(a.begin(), a.end(), out);
}

void ab_free(void* h) { delete static_cast<Built*>(h); }

}
