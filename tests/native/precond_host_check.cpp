// Host shim of tests/test_precond_setup_host.py: builds a Layout with the calls handle creation makes
// (fvhip_api.cpp createCtx: topoFromMesh, or partitionRCB + extractPartition with a two-layer halo, then
// buildLayout), runs the preconditioners' structure builders of precond_setup.cpp and the coarsening loop of
// fvhip_ctx::ensureAmg on it, and hands the arrays out. No device is touched.
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
	std::vector<std::vector<int>> arrays;      // indexed as the test's constants (SCALARS, LINE_START, ...)
};
constexpr int LEVEL0 = 16;
}

extern "C" {

const char* pc_error() { return g_error.c_str(); }

void* pc_build(const fvhip_mesh* mesh, const fvhip_flow_config* cfg, int nparts, int rank, double line_thr,
               int amg_levels, double amg_thr)
{
	try {
		Layout L;
		if(nparts > 1) {
			const std::vector<int> part = partitionRCB(mesh->rc, mesh->nelem, nparts);
			L = buildLayout(extractPartition(*mesh, part.data(), rank, 2), *cfg, true);
		} else L = buildLayout(topoFromMesh(*mesh), *cfg, true);
		const CellGraph G = cellGraph(L);
		const Colouring C = colourCells(G);
		const LinePlan P = buildLines(G, line_thr);
		std::vector<AmgLevelHost> levels;
		AmgGraph g = amgFineGraph(G);
		for(int l = 1; l < amg_levels; l++) {            // fvhip_ctx::ensureAmg's loop and stop rules
			if(g.n < 64) break;
			AmgLevelHost H = amgCoarsen(g, amg_thr);
			if(H.n*5 > g.n*4) break;
			g = amgGraphOf(H);
			levels.push_back(std::move(H));
		}
		Built* B = new Built();
		B->arrays.resize(LEVEL0 + 3*levels.size());
		B->arrays[0] = {L.ncell, L.nghost, static_cast<int>(C.triples), static_cast<int>(levels.size()),
		                P.twisted_groups, P.nlines, P.ngroups, P.nrows};
		B->arrays[1] = P.line_start; B->arrays[2] = P.line_cells; B->arrays[3] = P.line_faces;
		B->arrays[4] = C.colour; B->arrays[5] = C.colour_start;
		B->arrays[6].assign(C.cells.begin(), C.cells.begin() + L.ncell);
		B->arrays[7] = L.if_L; B->arrays[8] = L.if_R;
		B->arrays[9] = P.gstart; B->arrays[10] = P.cell; B->arrays[11] = P.face; B->arrays[12] = P.len;
		B->arrays[13].assign(L.perm.begin(), L.perm.begin() + L.ncell);   // what fvhip_get_permutation hands out
		for(size_t l = 0; l < levels.size(); l++) {
			B->arrays[LEVEL0 + 3*l] = levels[l].agg;
			B->arrays[LEVEL0 + 3*l + 1] = levels[l].rowptr;
			B->arrays[LEVEL0 + 3*l + 2] = levels[l].col;
		}
		return B;
	} catch(const std::exception& e) {
		g_error = e.what();
		return nullptr;
	}
}

long long pc_size(void* h, int what)
{
	const Built* B = static_cast<const Built*>(h);
	return what >= 0 && what < static_cast<int>(B->arrays.size()) ? static_cast<long long>(B->arrays[what].size()) : 0;
}

void pc_copy(void* h, int what, int* out)
{
	const std::vector<int>& a = static_cast<const Built*>(h)->arrays[static_cast<size_t>(what)];
	std::copy(a.begin(), a.end(), out);
}

void pc_free(void* h) { delete static_cast<Built*>(h); }

}
