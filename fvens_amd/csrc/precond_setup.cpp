/** \file precond_setup.cpp
 * \brief The preconditioners' structures from the Layout (precond_setup.hpp). Everything is built in a
 *   fixed order, so a mesh gives the same lines, colours and graphs on every run.
 */
#include "precond_setup.hpp"
#include "layout.hpp"

#include <algorithm>
#include <cmath>
#include <deque>
#include <numeric>
#include <stdexcept>
#include <utility>

namespace fvhip {

CellGraph cellGraph(const Layout& L)
{
	CellGraph G;
	G.ncell = L.ncell; G.ninface = L.ninface;
	G.nbr.resize(static_cast<size_t>(L.ncell));
	for(int c = 0; c < L.ncell; c++)
		for(int j = 0; j < 4; j++) {
			const int code = L.cell_rfaces[4*static_cast<size_t>(c)+j];
			if(code < 0 || (code >> 1) < L.nbface) continue;          // padding, boundary face
			CellGraph::Nbr& b = G.nbr[c][j];
			b.cell = L.cell_nbr_fo[4*static_cast<size_t>(c)+j];
			b.fi = (code >> 1) - L.nbface;
			b.right = (code & 1) != 0;
			const double dx = L.rc[2*static_cast<size_t>(c)] - L.rc[2*static_cast<size_t>(b.cell)];
			const double dy = L.rc[2*static_cast<size_t>(c)+1] - L.rc[2*static_cast<size_t>(b.cell)+1];
			b.w = L.if_len[b.fi]/std::sqrt(dx*dx + dy*dy);
		}
	return G;
}

Colouring colourCells(const CellGraph& G)
{
	const int N = G.ncell;
	auto nbr = [&](int c, int j) { return G.owned(G.nbr[c][j]) ? G.nbr[c][j].cell : -1; };
	Colouring C;
	for(int c = 0; c < N; c++)
		for(int j = 0; j < 4; j++) {
			const int a = nbr(c, j);
			if(a <= c) continue;
			for(int k = j + 1; k < 4; k++) {
				const int b = nbr(c, k);
				if(b <= c) continue;
				for(int m = 0; m < 4; m++) if(nbr(a, m) == b) C.triples++;
			}
		}
	const AmgGraph g = amgFineGraph(G);               // the owned cells' adjacency
	C.colour = greedyColouring(g.rowptr, g.col, C.colour_start, C.cells);
	C.cells.resize(std::max<size_t>(C.cells.size(), 1));
	return C;
}

IluOrder iluOrder(const CellGraph& G, int order)
{
	if(order != 1 && order != 2) throw std::invalid_argument("ilu_order must be 1 (internal order) or 2 (reverse Cuthill-McKee)");
	const int N = G.ncell;
	IluOrder O;
	O.rank.resize(static_cast<size_t>(N));
	std::iota(O.rank.begin(), O.rank.end(), 0);
	// owned neighbours of every cell, ascending id, and their count (the degree)
	std::vector<std::array<int,4>> nb(static_cast<size_t>(N));
	std::vector<int> deg(static_cast<size_t>(N), 0);
	for(int c = 0; c < N; c++) {
		for(const CellGraph::Nbr& b : G.nbr[c]) if(G.owned(b)) nb[c][deg[c]++] = b.cell;
		std::sort(nb[c].begin(), nb[c].begin() + deg[c]);
	}
	if(order == 2) {
		std::vector<int> dist(static_cast<size_t>(N), -1), queue, list;
		queue.reserve(static_cast<size_t>(N)); list.reserve(static_cast<size_t>(N));
		auto bfs = [&](int root, bool sorted) {          // fills queue with root's component; returns the last cell reached
			queue.clear();
			dist[root] = 0; queue.push_back(root);
			for(size_t q = 0; q < queue.size(); q++) {
				const int a = queue[q];
				const size_t first = queue.size();
				for(int j = 0; j < deg[a]; j++) {
					const int k = nb[a][j];
					if(dist[k] < 0) { dist[k] = dist[a] + 1; queue.push_back(k); }
				}
				if(sorted) std::sort(queue.begin() + first, queue.end(), [&](int x, int y) {
					return deg[x] != deg[y] ? deg[x] < deg[y] : x < y; });
			}
			return queue.back();
		};
		std::vector<char> done(static_cast<size_t>(N), 0);
		for(int seed = 0; seed < N; seed++) {
			if(done[seed]) continue;
			int root = seed;
			for(int rep = 0; rep < 2; rep++) {           // pseudo-peripheral cell of this component
				const int far = bfs(root, false);
				for(const int a : queue) dist[a] = -1;
				root = far;
			}
			bfs(root, true);
			for(const int a : queue) { done[a] = 1; list.push_back(a); }
		}
		for(int p = 0; p < N; p++) O.rank[list[static_cast<size_t>(N - 1 - p)]] = p;
	}
	// longest chain of lower links: cells in rank order, each one longer than its longest lower neighbour's
	std::vector<int> at(static_cast<size_t>(N)), len(static_cast<size_t>(N), 0);
	for(int c = 0; c < N; c++) at[O.rank[c]] = c;
	for(int p = 0; p < N; p++) {
		const int c = at[p];
		int l = 0;
		for(int j = 0; j < deg[c]; j++) if(O.rank[nb[c][j]] < p) l = std::max(l, len[nb[c][j]]);
		len[c] = l + 1;
		O.depth = std::max(O.depth, len[c]);
	}
	return O;
}

namespace {

typedef std::vector<std::pair<int,int>> Line;     ///< (cell, interior face to the previous entry; -1 at the first)

/// lines in discovery order, cut at LINE_MAX_CELLS
std::vector<Line> growLines(const CellGraph& G, double thr)
{
	const int N = G.ncell;
	// per cell: its owned neighbours, strongest first (equal couplings: lower cell first), and the ratio of
	// its strongest to its weakest coupling over all interior faces
	std::vector<std::array<CellGraph::Nbr,4>> nbr(static_cast<size_t>(N));
	std::vector<int> nn(static_cast<size_t>(N), 0);
	std::vector<double> ratio(static_cast<size_t>(N), 1.0);
	for(int c = 0; c < N; c++) {
		double wmax = 0, wmin = INFINITY;
		for(const CellGraph::Nbr& b : G.nbr[c]) {
			if(b.cell < 0) continue;
			wmax = std::max(wmax, b.w); wmin = std::min(wmin, b.w);
			if(G.owned(b)) nbr[c][nn[c]++] = b;
		}
		std::sort(nbr[c].begin(), nbr[c].begin() + nn[c], [](const CellGraph::Nbr& a, const CellGraph::Nbr& b) {
			return a.w > b.w || (a.w == b.w && a.cell < b.cell); });
		if(wmin < INFINITY && wmin > 0) ratio[c] = wmax/wmin;
	}
	auto strong2 = [&](int c, int o) {               // o among c's two strongest owned neighbours
		for(int j = 0; j < std::min(nn[c], 2); j++) if(nbr[c][j].cell == o) return true;
		return false;
	};
	std::vector<int> order(static_cast<size_t>(N));
	std::iota(order.begin(), order.end(), 0);
	std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ratio[a] > ratio[b]; });
	std::vector<char> used(static_cast<size_t>(N), 0);
	std::vector<Line> all;
	for(const int c0 : order) {
		if(used[c0]) continue;
		used[c0] = 1;
		std::deque<std::pair<int,int>> line{{c0, -1}};
		if(ratio[c0] >= thr) {
			for(int dir = 0; dir < 2; dir++) {
				int e = dir == 0 ? line.back().first : line.front().first;
				for(;;) {
					int nxt = -1, fi = -1;
					for(int j = 0; j < std::min(nn[e], 2); j++) {
						const CellGraph::Nbr& b = nbr[e][j];
						if(!used[b.cell]) { nxt = b.cell; fi = b.fi; break; }
					}
					if(nxt < 0 || ratio[nxt] < thr || !strong2(nxt, e)) break;
					used[nxt] = 1;
					if(dir == 0) line.push_back({nxt, fi});
					else {                              // prepend: the face now links nxt to e
						line.front().second = fi;
						line.push_front({nxt, -1});
					}
					e = nxt;
				}
			}
		}
		// lines longer than LINE_MAX_CELLS are cut into pieces: the recurrence along a line is
		// sequential, so one line of thousands of cells (circumferential lines of the outer O-grid
		// layers) would set the whole sweep's time
		for(size_t b = 0; b < line.size(); b += LINE_MAX_CELLS) {
			const size_t e = std::min(line.size(), b + static_cast<size_t>(LINE_MAX_CELLS));
			Line piece(line.begin() + b, line.begin() + e);
			piece[0].second = -1;
			all.push_back(std::move(piece));
		}
	}
	return all;
}

/// the stored code of interior face fi leading to line cell c: fi << 1 | (the previous cell is its R; walking
/// the other way it is c: the code with its low bit flipped)
int faceCode(const CellGraph& G, int c, int fi)
{
	for(const CellGraph::Nbr& b : G.nbr[c]) if(b.fi == fi) return (fi << 1) | (b.right ? 0 : 1);
	throw std::logic_error("buildLines: a line crosses a face its cell does not have");
}

}

LinePlan buildLines(const CellGraph& G, double thr)
{
	std::vector<Line> all = growLines(G, thr);
	// longest first; lines of equal length in ascending internal (Hilbert) order of their first cell, so
	// that the 64 lanes of a group walk neighbouring lines side by side: their k-th cells' rows of v and
	// z share 128-byte lines (the cells are gathered by index), instead of 64 unrelated places of the mesh.
	// Each line's recurrence is independent of the lane it runs on: the same z bit for bit.
	std::stable_sort(all.begin(), all.end(), [](const Line& a, const Line& b) {
		return a.size() > b.size() || (a.size() == b.size() && a[0].first < b[0].first); });
	// from here an entry's face is its stored code
	for(Line& ln : all) for(size_t k = 1; k < ln.size(); k++) ln[k].second = faceCode(G, ln[k].first, ln[k].second);
	// lanes: a line of at least LINE_TWIST_MIN cells is solved from both ends (twisted factorisation):
	// its top half t = (n-1)/2 cells in order, then the twist cell t, on lane j of a twisted group; its
	// bottom half n-1 .. t+1 in reverse order, then t, on lane j+32. Every other line is one lane of a
	// group of 64. Rows line-interleaved (lines.hpp LineSet)
	const int nl = static_cast<int>(all.size());
	int ntw = 0;
	while(ntw < nl && static_cast<int>(all[static_cast<size_t>(ntw)].size()) >= LINE_TWIST_MIN) ntw++;
	std::vector<std::array<Line,64>> grp;
	for(int l0 = 0; l0 < ntw; l0 += 32) {
		grp.emplace_back();
		for(int q = 0; q < 32 && l0 + q < ntw; q++) {
			const Line& ln = all[static_cast<size_t>(l0 + q)];
			const int n = static_cast<int>(ln.size()), tc = (n - 1)/2;
			Line top(ln.begin(), ln.begin() + tc + 1), bot;
			for(int k = n - 1; k >= tc; k--)
				bot.push_back({ln[static_cast<size_t>(k)].first, k == n - 1 ? -1 : ln[static_cast<size_t>(k) + 1].second ^ 1});
			grp.back()[static_cast<size_t>(q)] = std::move(top);
			grp.back()[static_cast<size_t>(q) + 32] = std::move(bot);
		}
	}
	LinePlan P;
	P.twisted_groups = static_cast<int>(grp.size());
	for(int l0 = ntw; l0 < nl; l0 += 64) {
		grp.emplace_back();
		for(int q = 0; q < 64 && l0 + q < nl; q++) grp.back()[static_cast<size_t>(q)] = all[static_cast<size_t>(l0 + q)];
	}
	const int ng = static_cast<int>(grp.size());
	P.nlines = nl;
	P.ngroups = ng;
	P.gstart.assign(static_cast<size_t>(ng) + 1, 0);
	for(int g = 0; g < ng; g++) {
		size_t mx = 0;
		for(const Line& ln : grp[static_cast<size_t>(g)]) mx = std::max(mx, ln.size());
		P.gstart[g+1] = P.gstart[g] + static_cast<int>(mx);
	}
	P.nrows = P.gstart[ng];
	const size_t nslot = 64*static_cast<size_t>(P.nrows);
	P.cell.assign(std::max<size_t>(nslot, 1), -1);
	P.face.assign(std::max<size_t>(nslot, 1), -1);
	P.len.assign(std::max<size_t>(64*static_cast<size_t>(ng), 1), 0);
	for(int g = 0; g < ng; g++)
		for(size_t lane = 0; lane < 64; lane++) {
			const Line& ln = grp[static_cast<size_t>(g)][lane];
			P.len[64*static_cast<size_t>(g) + lane] = static_cast<int>(ln.size());
			for(size_t k = 0; k < ln.size(); k++) {
				const size_t slot = (static_cast<size_t>(P.gstart[g]) + k)*64 + lane;
				P.cell[slot] = ln[k].first;
				P.face[slot] = ln[k].second;
			}
		}
	// the lines as built, longest first
	P.line_start.assign(1, 0);
	for(const Line& ln : all) {
		for(const auto& e : ln) { P.line_cells.push_back(e.first); P.line_faces.push_back(e.second); }
		P.line_start.push_back(static_cast<int>(P.line_cells.size()));
	}
	return P;
}

AmgGraph amgFineGraph(const CellGraph& G)
{
	const int N = G.ncell, Fi = G.ninface;
	std::vector<std::vector<AmgEntry>> rows(static_cast<size_t>(N));
	for(int c = 0; c < N; c++)
		for(const CellGraph::Nbr& b : G.nbr[c])
			if(G.owned(b)) rows[c].push_back({b.cell, b.w, b.right ? N + b.fi : N + Fi + b.fi});   // A[c][o]: c = R reads lower, c = L upper
	return amgGraphOfRows(rows);
}

}
