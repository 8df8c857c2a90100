/** \file precond_setup.hpp
 * \brief Host structure builders of the preconditioners (precond_setup.cpp, amg.cpp): the owned cells' graph
 *   over interior faces, the multicolour order, the lines and their 64-lane packing, the multigrid's graphs
 *   and coarse levels. Pure functions of the Layout -- no device, no handle (fvhip_ctx::ensureColouring /
 *   ensureLines / ensureAmg upload what they return) -- so they run in CPU tests. The options
 *   that select among them: precond_options.hpp.
 */
#ifndef FVHIP_PRECOND_SETUP_HPP
#define FVHIP_PRECOND_SETUP_HPP

#include <array>
#include <vector>

namespace fvhip {

struct Layout;

#ifndef FVHIP_LINE_MAX
#define FVHIP_LINE_MAX 256
#endif
constexpr int LINE_MAX_CELLS = FVHIP_LINE_MAX;   ///< longest line piece (buildLines)
#ifndef FVHIP_LINE_TWIST_MIN
#define FVHIP_LINE_TWIST_MIN 16
#endif
constexpr int LINE_TWIST_MIN = FVHIP_LINE_TWIST_MIN;   ///< shortest line solved from both ends

/// The owned cells' neighbours across their faces (slots in ascending reference face index): the one decoder
/// of Layout::cell_rfaces / cell_nbr_fo
struct CellGraph
{
	struct Nbr {
		int cell = -1;        ///< internal id across an interior face (>= ncell: a ghost); -1: boundary face or padding
		int fi = -1;          ///< the interior face (index into Layout::if_*)
		bool right = false;   ///< the cell is the face's right cell
		double w = 0.0;       ///< coupling: face length / centre distance (what dominates the blocks of thin cells)
	};
	int ncell = 0, ninface = 0;
	std::vector<std::array<Nbr,4>> nbr;   ///< [ncell][4]
	bool owned(const Nbr& b) const { return b.cell >= 0 && b.cell < ncell; }
};
CellGraph cellGraph(const Layout& L);

/// Greedy colouring of the owned cells in internal (Hilbert) order over interior faces; ghost cells are not
/// coloured (within a sweep they hold the values of the last exchange)
struct Colouring
{
	std::vector<int> colour;                 ///< [ncell], also the ILU(0) order
	std::vector<int> colour_start, cells;    ///< cells of colour q = cells[colour_start[q] ..], ascending
	long long triples = 0;                   ///< owned cells sharing faces pairwise three at a time (ILU(0) fill off the diagonal)
};
Colouring colourCells(const CellGraph& G);

/// A total order of the owned cells for the sweep-based ILU(0)/SGS (fvhip_implicit_config::ilu_order): owned
/// neighbour k of cell i across an interior face is `lower` if rank[k] < rank[i], else `upper`.
///   order 1: the internal (Hilbert) order, rank[c] = c.
///   order 2: reverse Cuthill-McKee of the owned cells' interior-face graph (the reference's -mesh_reorder rcm):
///     connected components in ascending lowest internal id, each started at a pseudo-peripheral cell (the
///     farthest of the farthest of its lowest cell, partition.cpp's search), breadth-first with the unvisited
///     neighbours taken in ascending (degree, id), the whole list reversed.
/// depth = cells of the longest chain of lower-neighbour links: with depth - 1 build sweeps the pivots are the
/// sequential factorisation's, with depth apply sweeps the triangular solves are exact.
struct IluOrder
{
	std::vector<int> rank;                   ///< [ncell]: position of each owned cell in the order
	int depth = 0;
};
IluOrder iluOrder(const CellGraph& G, int order);

/// Lines of the line-implicit preconditioner. A cell is anisotropic if its strongest coupling (ghost
/// neighbours included) is at least `thr` times its weakest; lines start at the most anisotropic unassigned
/// cell and grow at both ends through the end cell's strongest unassigned owned neighbour while that
/// neighbour is anisotropic and the link is one of its own two strongest (Mavriplis' line construction);
/// every other cell is a line of one. Lines are cut at LINE_MAX_CELLS and sorted by length, so that a wave's
/// threads walk lines of similar length.
struct LinePlan
{
	/// the lines as built: cells of line l = line_cells[line_start[l] ..], line_faces = interior face to the
	/// previous cell, fi << 1 | (previous cell is its R), -1 at a line's first cell
	std::vector<int> line_start, line_cells, line_faces;
	/// the same dealt to groups of 64 lanes (lines.hpp LineSet)
	int twisted_groups = 0, nlines = 0, ngroups = 0, nrows = 0;
	std::vector<int> gstart, cell, face, len;
};
LinePlan buildLines(const CellGraph& G, double thr);

/// one coarse level of the aggregation multigrid as built on the host (amg.hpp)
struct AmgLevelHost
{
	int n = 0;                               ///< block rows
	std::vector<int> rowptr, col, dpos;      ///< block CSR (columns ascending, diagonal included; dpos = its position)
	std::vector<int> cstart, csrc;           ///< per nonzero: contributing blocks of the finer level (ascending)
	std::vector<int> mstart, members;        ///< per row: the finer level's rows aggregated into it (ascending)
	std::vector<int> agg;                    ///< per row of the finer level: its aggregate (row of this level)
	std::vector<int> cstart_colour, cells;   ///< multicolour order: rows of colour q = cells[cstart_colour[q]..]
	std::vector<double> w;                   ///< coupling per nonzero (aggregation of the next level)
};

/// the finer level seen by the aggregation: rows, adjacency with couplings (symmetric), and the block index
/// of each nonzero of the finer operator (finest: diag c -> c, A[R][L] = lower fi -> n + fi, A[L][R] = upper
/// fi -> n + Fi + fi; coarse: the CSR position)
struct AmgGraph
{
	int n = 0;
	std::vector<int> rowptr, col;            ///< off-diagonal adjacency, columns ascending
	std::vector<double> w;                   ///< coupling per adjacency entry
	std::vector<int> blk;                    ///< block index of A[row][col] per adjacency entry
	std::vector<int> dblk;                   ///< block index of A[row][row]
};

/// one adjacency entry of a graph under construction; rows are ordered by column, then coupling, then block
struct AmgEntry
{
	int col; double w; int blk;
	bool operator<(const AmgEntry& o) const { return col != o.col ? col < o.col : w != o.w ? w < o.w : blk < o.blk; }
};
/// the graph of the given rows (each sorted here); row c's diagonal block index is c
AmgGraph amgGraphOfRows(std::vector<std::vector<AmgEntry>>& rows);
/// the finest level's graph: the owned cells over interior faces (ghost couplings dropped: block-Jacobi
/// across ranks), block indices those of the face-ordered Jacobian
AmgGraph amgFineGraph(const CellGraph& G);
/// aggregates graph g (threshold: strength relative to both cells' strongest coupling) and builds the
/// coarse level: pattern, Galerkin contribution lists, member lists, colouring, coarse couplings
AmgLevelHost amgCoarsen(const AmgGraph& g, double threshold);
/// the block smoother's view of a level's colour order (cstart_colour / cells of amgCoarsen, n rows) cut into
/// contiguous row blocks of R rows: off[(nb + 1) * nc], nb = ceil(n / R) blocks and nc colours; the rows of
/// colour q in block k are cells[off[k nc + q] .. off[(k+1) nc + q]) -- a sub-range of the colour's list, which
/// ascends (found by binary search); empty where the block has no row of the colour. R >= 1
std::vector<int> amgBlockOffsets(int n, const std::vector<int>& cstart_colour, const std::vector<int>& cells, int R);
/// the graph of a built coarse level (for the next aggregation)
AmgGraph amgGraphOf(const AmgLevelHost& L);
/// greedy colouring of a CSR adjacency in row order (a diagonal entry is skipped): the colours, and the rows
/// colour by colour (colour q = rows[start[q] ..], ascending)
std::vector<int> greedyColouring(const std::vector<int>& rowptr, const std::vector<int>& col, std::vector<int>& start,
                                 std::vector<int>& rows);

}
#endif
