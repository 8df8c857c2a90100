/** \file ctx.hpp
 * \brief The library handle (struct fvhip_ctx behind include/fvhip.h's fvhip_handle): its state -- device mesh,
 *   state scratch, Jacobian, the work space of the implicit solver -- the profiling helpers and the short
 *   predicates, and the declarations of what works on it: the allocators, surface cache and single-domain
 *   matrix-free operator (ctx.cpp), the halo transport (halo_exchange.cpp), the residual stages (residual.cpp)
 *   and the preconditioner structures (precond.cpp). Shared by every host translation unit.
 * No exception crosses the ABI: entry points wrap their bodies in guard().
 */
#ifndef FVHIP_CTX_HPP
#define FVHIP_CTX_HPP

#include "../../include/fvhip.h"
#include "layout.hpp"
#include "kernels.hpp"
#include "jacobian.hpp"
#include "blockops.hpp"
#include "lines.hpp"
#include "mesh.hpp"
#include "partition.hpp"
#include "halo.hpp"
#include "halo_legs.hpp"
#include "ode.hpp"
#include "surface.hpp"
#include "amg.hpp"
#include <rccl/rccl.h>
#include <hip/hip_runtime.h>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include <map>
#include <stdexcept>
#include <memory>
#include <array>

#include "krylov.hpp"

namespace fvhip_detail {

inline thread_local std::string g_err;      ///< fvhip_last_error() text, shared by every TU

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };

inline void hipCheck(hipError_t e, const char* what) {
	if(e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e));
}
#define HC(x) hipCheck((x), #x)

inline void ncclCheck(ncclResult_t e, const char* what) {
	if(e != ncclSuccess) throw std::runtime_error(std::string(what) + ": " + ncclGetErrorString(e));
}
#define NC(x) ncclCheck((x), #x)

template <typename F>
inline int guard(F&& f) {
	try { f(); return 0; }
	catch(const std::exception& e) { g_err = e.what(); return 1; }
	catch(...) { g_err = "unknown error"; return 1; }
}

/// entry-point argument check: a null handle or a null array the call reads or writes is refused
/// with "null <what>" before any host or device access (a null device pointer would fault the GPU)
inline void need(const void* p, const char* what) {
	if(!p) throw std::invalid_argument(std::string("null ") + what);
}

/// the same for a group call's per-rank arrays: the array of pointers and each rank's entry
template <typename T>
inline void needEach(T* const* p, size_t n, const char* what) {
	need(p, what);
	for(size_t i = 0; i < n; i++) need(p[i], what);
}

/// the same for a call's Jacobian blocks: the diagonal, and the face blocks where the handle has interior faces
inline void needBlocks(int ninface, const void* diag, const void* lower, const void* upper) {
	need(diag, "diag");
	if(ninface > 0) { need(lower, "lower"); need(upper, "upper"); }
}

template <typename T>
inline T* upload(const std::vector<T>& v, std::vector<void*>& owned) {
	if(v.empty()) return nullptr;
	void* p = nullptr;
	HC(hipMalloc(&p, v.size()*sizeof(T)));
	HC(hipMemcpy(p, v.data(), v.size()*sizeof(T), hipMemcpyHostToDevice));
	owned.push_back(p);
	return static_cast<T*>(p);
}

inline double* dalloc(size_t n, std::vector<void*>& owned) {
	if(n == 0) n = 1;
	void* p = nullptr;
	HC(hipMalloc(&p, n*sizeof(double)));
	owned.push_back(p);
	return static_cast<double*>(p);
}

/// interleave int pairs / 4-tuples for vector loads
inline std::vector<int> pack2(const std::vector<int>& a, const std::vector<int>& b) {
	std::vector<int> o(2*a.size());
	for(size_t i = 0; i < a.size(); i++) { o[2*i] = a[i]; o[2*i+1] = b[i]; }
	return o;
}

}

using namespace fvhip;
using namespace fvhip_detail;

/// which residual a call asks for: the configuration's best (fused where it applies), the staged gradient +
/// sweep sequence, its pipelined form, or the fused one with the ghost rows of u already current
enum class ResidualPath { Default, Staged, Pipelined, HaloReady };

/// operands of the matrix-free operator fused into the residual kernel (fvhip_ctx::stage_fused)
struct MfFuse { const double *x = nullptr, *pm = nullptr, *res = nullptr, *mdt = nullptr; };

struct fvhip_ctx
{
	int device = 0;
	hipStream_t stream = nullptr;
	fvhip_flow_config cfg{};
	std::vector<int> bc_type, bc_tag;
	std::vector<double> bc_vals;
	Layout L;
	DevMesh M{};
	DevPhys P{};
	std::vector<void*> owned;
	int* d_perm = nullptr;
	// state scratch
	double *d_u = nullptr, *d_up = nullptr, *d_grad = nullptr, *d_lgrad = nullptr, *d_phi = nullptr;
	double *d_ubc = nullptr, *d_ug = nullptr, *d_r = nullptr, *d_dtm = nullptr;
	// mat-free state
	double *d_mf_u = nullptr, *d_mf_r = nullptr, *d_mf_mdt = nullptr, *d_mf_aux = nullptr, *d_mf_y = nullptr;
	double mf_eps = 1e-7;
	const double *mf_u = nullptr, *mf_r = nullptr, *mf_mdt = nullptr;   // device state of the operator
	double *d_part = nullptr, *d_pm = nullptr;
	double* d_stage = nullptr;                       // Runge-Kutta stage state (owned + ghost rows: SSP-RK's is a residual's input)
	/// BDF dual time (implicit.cpp dualTime), owned rows each: the states u^n and u^(n-1), whose pointers trade
	/// places at the start of a step, and the unsteady residual G (d_r stays the spatial residual: the matrix-free
	/// operator differences it)
	double *d_bdf_n = nullptr, *d_bdf_m = nullptr, *d_bdf_g = nullptr;
	double* d_ent = nullptr;                        // entropy-error partial sums (fvhip_entropy_error_device)
	/// work space of the implicit solver (implicit.cpp), allocated on first use
	struct ImplicitWork {
		int m = 0;                                  ///< GMRES restart length the basis holds
		double* V = nullptr;                        ///< Krylov basis [m+1][4*ncell]
		double *z = nullptr, *aux = nullptr;        ///< [4*(ncell+nghost)]: operator inputs (ghost rows)
		double *w = nullptr, *t = nullptr, *s = nullptr, *du = nullptr, *yg = nullptr;   ///< [4*ncell]
		double *jd = nullptr, *jlo = nullptr, *jup = nullptr, *dinv = nullptr;            ///< 4x4 blocks
		float *slo = nullptr, *sup = nullptr, *sdinv = nullptr;   ///< fp32 copies for the preconditioner
		float* sdiag = nullptr;                     ///< fp32 diagonal blocks (the multigrid's finest residuals)
		double *part = nullptr, *red = nullptr, *coef = nullptr, *pm = nullptr;           ///< reductions
		double *h_red = nullptr, *h_coef = nullptr, *h_red2 = nullptr;                  ///< pinned host
	} iw;
	std::vector<void*> owned_host;                  ///< pinned host allocations
	// Jacobian
	JacMesh J{};
	bool jac_ready = false;
	double *d_jb = nullptr, *d_jlo = nullptr, *d_jup = nullptr, *d_jdiag = nullptr;
	/// reference-order rows of the host-pointer entries (fvhip_compute_residual & co.): the host array is
	/// copied as it is and reordered on the device (k_gather / k_scatter over d_perm)
	double* d_raw = nullptr;
	size_t raw_cap = 0;
	double* rawScratch(size_t doubles);
	// partitioned meshes: halo exchange with the neighbour ranks (RCCL, or in-process for a group)
	int rank = 0, nparts = 1;
	bool rankmesh = false;        ///< one rank's subdomain with connectivity faces (fvhip_create, nconnface > 0)
	/// periodic handle: every connectivity face names rank -1, the mesh itself (makePeriodic). Rank 0 of 1; the
	/// exchanges are gathers on the device (k_ghost_gather), no communicator or group is needed
	bool periodic = false;
	int* d_trace_from = nullptr;  ///< periodic handles: [nconnface] the partner's connectivity face
	// pipelined staged residual (single domain): the sweep groups run on stream2 behind the
	// gradient chunks of `stream`
	int* d_pipe_patch = nullptr;
	hipStream_t stream2 = nullptr;
	std::vector<hipEvent_t> pipe_ev;
	hipEvent_t pipe_start = nullptr, pipe_done = nullptr;
	ncclComm_t comm = nullptr;
	bool in_group = false;
	// halo exchange overlapped with the interior patches of the fused residual (RCCL handles)
	int* d_fz_order = nullptr;
#ifdef FVHIP_FZ_STAMPS
	unsigned long long* d_stamps = nullptr;   ///< probe build: the last fused launch's stamps (fused.hip FzStamps)
	long long stamp_blocks = 0;               ///< blocks of that launch
#endif
	hipStream_t comm_stream = nullptr;
	hipEvent_t ev_u = nullptr, ev_halo = nullptr;
	hipEvent_t ev_packed = nullptr, ev_copied = nullptr;   ///< in-process overlapped transport (groups)
	bool copied_recorded = false;
	int* d_send = nullptr;
	int* d_border = nullptr;
	int nborder = 0;
	double* d_sendbuf = nullptr;
	int* d_trace_conn = nullptr;     ///< per-rank meshes: Layout::trace_conn on the device
	double* d_tracebuf = nullptr;    ///< [nghost][4] received face traces before the unpack
	int nsend = 0;
	// profiling
	bool prof = false;
	struct Rec { std::string name; hipEvent_t a, b; };
	std::vector<Rec> recs;
	std::map<std::string, std::pair<double,int>> acc;

	~fvhip_ctx() {
		(void)hipSetDevice(device);
		if(comm) (void)ncclCommDestroy(comm);
		for(auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
		for(hipEvent_t e : pipe_ev) (void)hipEventDestroy(e);
		if(pipe_start) (void)hipEventDestroy(pipe_start);
		if(pipe_done) (void)hipEventDestroy(pipe_done);
		if(stream2) (void)hipStreamDestroy(stream2);
		if(ev_u) (void)hipEventDestroy(ev_u);
		if(ev_halo) (void)hipEventDestroy(ev_halo);
		if(ev_packed) (void)hipEventDestroy(ev_packed);
		if(ev_copied) (void)hipEventDestroy(ev_copied);
		if(comm_stream) (void)hipStreamDestroy(comm_stream);
		for(void* p : owned) (void)hipFree(p);
		for(void* p : owned_host) (void)hipHostFree(p);
		if(stream) (void)hipStreamDestroy(stream);
	}

	template <typename F>
	void timed(const std::string& name, F&& launch) { timed_on(stream, name, launch); }
	template <typename F>
	void timed_on(hipStream_t st, const std::string& name, F&& launch) {
		if(!prof) { launch(); return; }
		Rec r; r.name = name;
		HC(hipEventCreate(&r.a)); HC(hipEventCreate(&r.b));
		HC(hipEventRecord(r.a, st));
		launch();
		HC(hipEventRecord(r.b, st));
		recs.push_back(r);
	}
	void collect() {
		HC(hipStreamSynchronize(stream));
		for(auto& r : recs) {
			float ms = 0;
			HC(hipEventElapsedTime(&ms, r.a, r.b));
			auto& a = acc[r.name]; a.first += ms; a.second += 1;
			(void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
		}
		recs.clear();
	}

	/// kernels of the selected numerics mode (exact: bitwise parity; fast: stated tolerance)
#define KOPS(fn) (cfg.fast_math ? fast::fn : exact::fn)
	int recKind() const {
		if(!cfg.order2) return SR_FIRST;
		return cfg.reconstruction == FVHIP_REC_VANALBADA ? SR_MUSCL : SR_LINEAR;
	}
	int viscKind() const {
		if(!cfg.viscous_sim) return SV_NONE;
		return cfg.const_visc ? SV_CONST : SV_SUTHERLAND;
	}

	bool halo() const { return !L.nbr_rank.empty(); }
	/// a handle with ghost rows that nothing fills yet: partitioned, without its communicator
	bool needsComm() const { return halo() && !comm && !periodic; }
	int ntotal() const { return L.ncell + L.nghost; }

	// --- residual stages (FlowFV::compute_residual, flow_spatial.cpp:636-816), residual.cpp; between them the
	// ghost rows of u, of the gradients and of limiter data are exchanged on partitioned meshes ---
	void stage_gradients(const double* u);
	bool limited() const {
		return cfg.reconstruction == FVHIP_REC_BARTHJESPERSEN || cfg.reconstruction == FVHIP_REC_VENKATAKRISHNAN;
	}
	/// WLS gradients compute the limiter in the same pass (k_prep_grad_wls<LIM>)
	bool fusedLimiter() const { return limited() && cfg.gradientscheme == FVHIP_GRAD_LEASTSQUARES; }
	void stage_limiter();
	void stage_weno();
	void stage_sweep(const double* u, double* r, bool dt, double* dtm, bool overwrite,
	                 const int* plist = nullptr, int pcount = 0, hipStream_t st = nullptr);
	void stage_border_gradients(const double* u, hipStream_t st = nullptr);
	void stage_ghost_gradients(const double* u, hipStream_t st = nullptr);
	/// mf: the operands of the matrix-free operator fused into the launch (below), else the plain residual
	void stage_fused(const double* u, double* r, bool dt, double* dtm, bool overwrite,
	                 const int* plist = nullptr, int pcount = 0, hipStream_t st = nullptr, const MfFuse& mf = MfFuse());

	/// one-launch residual (WLS + MUSCL / unlimited linear, inviscid)
	bool fused(ResidualPath p = ResidualPath::Default) const {
		return !L.fz_ext_start.empty() && (p == ResidualPath::Default || p == ResidualPath::HaloReady);
	}
	/// pipelined staged residual (single domain, WLS + MUSCL / unlimited linear, viscous too), on
	/// request only: on C4 it measured 0.55 ms against 0.46 ms for the serial staged path (the
	/// FP64-bound sweep groups and the HBM-bound gradient chunks slow each other down, and every
	/// group has its own tail)
	bool pipelined(ResidualPath p) const { return !L.pipe_cell_start.empty() && !halo() && p == ResidualPath::Pipelined; }
	void residual_pipelined(const double* u, double* r, bool dt, double* dtm, bool overwrite);

	/// the matrix-free operator fused into one launch of the residual kernel (single domain, fused
	/// configurations): y = mdt x + (r(u) - r(u + pm[1] x))/pm[1] with the perturbed state formed where the
	/// kernel reads a state row and the combination where it writes a cell -- k_mf_perturb's and
	/// k_mf_combine's arithmetic, so bitwise the three-launch operator, without its 5 vector passes over HBM
	/// (x and y must not alias: other blocks read x rows while a block writes its cells' y)
	bool matfreeFusable() const { return fused() && !halo(); }
	/// the fused operator's blocks read rows of x and of the state u that other blocks' cells need while each
	/// block writes its own cells of y: y must share no byte with x or u (else the three-launch operator runs)
	bool matfreeNoAlias(const double* u, const double* x, const double* y) const {
		const size_t n = 4*static_cast<size_t>(L.ncell), nt = 4*static_cast<size_t>(L.ncell + L.nghost);
		auto apart = [](const double* a, size_t na, const double* b, size_t nb) { return a + na <= b || b + nb <= a; };
		return apart(y, n, x, nt) && apart(y, n, u, nt);
	}

	// --- halo transport, halo_exchange.cpp ---
	/// pack the rows of `arr` (width doubles per cell) that the neighbours hold as ghosts
	void pack(const double* arr, int width, hipStream_t st = nullptr);
	/// L2TraceVector::updateSharedFacesBegin/End (tracevector.cpp:213-340) on a per-rank mesh: left
	/// [nconnface][width] holds this rank's face values of its connectivity faces (icface order); each
	/// neighbour's values of the same faces land in right[icface]. Packed in the exchange order (per
	/// neighbour rank, ascending global face), sent with RCCL, unpacked by face. width <= 4.
	void trace_pack(const double* left, int width, hipStream_t st);
	void trace_unpack(double* right, int width, hipStream_t st);
	void trace_exchange_rccl(const double* left, double* right, int width);
	/// exchange of the ghost rows of arr with every neighbour rank (RCCL; a periodic handle: a gather on its
	/// device), on stream st (default: the handle's); `layers` 2 fills both layers of a two-layer halo (the
	/// residual's state), 1 the first (gradients, limiter values, Krylov vectors)
	void exchange_rccl(double* arr, int width, hipStream_t st = nullptr, int layers = 1);
	/// the residual's halo protocol: with a two-layer halo and WLS gradients of an unlimited, MUSCL,
	/// Barth-Jespersen or Venkatakrishnan reconstruction, ONE exchange of u (both layers) and the
	/// layer-1 ghosts' gradients (and limiter values) computed locally (k_grad_ghost); otherwise u,
	/// then gradients (and limiter data) in further rounds
	bool singleExchange() const {
		return halo() && L.halo_layers == 2 && cfg.order2 && cfg.gradientscheme == FVHIP_GRAD_LEASTSQUARES &&
		       cfg.reconstruction != FVHIP_REC_WENO && (L.gg_cells.empty() || !L.gg_V.empty());
	}
	int limKind() const { return limited() ? (cfg.reconstruction == FVHIP_REC_VENKATAKRISHNAN ? 2 : 1) : 0; }
	/// the path fvhip_compute_residual_device's flags ask of this handle
	ResidualPath residualPath(int flags) const;
	/// the residual on this handle alone (fvhip_detail::residual over a system of one, residual.cpp)
	void residual(const double* u, double* r, bool dt, double* dtm, bool overwrite, ResidualPath path = ResidualPath::Default);

	// --- Jacobian, work space of the drivers, surface cache: ctx.cpp ---
	/// face-ordered mesh view and block buffers for the Jacobian, built on first use
	void ensureJacobian();
	/// Spatial::assemble_jacobian into (diag internal order, lower/upper reference face order); with
	/// cfl > 0 also the pseudo-time term (SteadyBackwardEulerSolver, aodesolver.cpp:300-329, 467) in the
	/// diagonal pass: dtm <- area/(cfl dtm), diag += dtm I
	void assemble(const double* u, double* diag, double* lower, double* upper, double cfl = 0.0, double* dtm = nullptr);
	/// reduction scratch of the device drivers (global sums, GMRES coefficients)
	void ensureReductions();
	/// operand buffers of the matrix-free operator and GMRES (ghost rows where an operator reads them)
	void ensureVectors();
	/// implicit-solver work space for GMRES(m): the above, the Jacobian blocks and the Krylov basis; m in
	/// [1, KRY_MAXK] (every caller has checked the restart length: PrecondOptions::check, fvhip_gmres_blocks_device)
	void ensureImplicit(int m);

	/// the boundary faces of one marker for the surface functionals, uploaded on first use
	struct SurfCache { SurfaceFaces S{}; double *faceout = nullptr, *contrib = nullptr, *sums = nullptr; };
	std::map<int, SurfCache> surf;
	SurfCache& surfaceFaces(int marker);

	/// multicolour order of block Gauss-Seidel (fvhip_implicit_config::prec_gs) and ILU(0), built on first use
	/// (precond_setup.hpp colourCells)
	std::vector<int> gs_colour_start;
	std::vector<int> gs_colour;          ///< colour of every owned cell (also the ILU(0) order)
	long long gs_triples = 0;            ///< owned cells sharing faces pairwise three at a time (ILU(0) fill off the diagonal)
	int *d_gs_cells = nullptr, *d_gs_colour = nullptr;
	void ensureColouring();                  // the preconditioner's methods, here to ensureSinglePrecond: precond.cpp
	/// block ILU(0) factorisation in colour order (fvhip_implicit_config::prec_ilu): dinv = the inverted
	/// pivot blocks Dt^-1, colour after colour (each colour reads the earlier colours' pivots)
	void iluFactor(const double* diag, const double* lower, const double* upper, double* dinv, hipStream_t st = nullptr);

	/// row orders of the sweep-based block ILU(0)/SGS (fvhip_implicit_config::ilu_order 1, 2), built on first use
	/// (precond_setup.hpp iluOrder); d_rank stays null for order 1 (the kernels compare cell indices)
	struct IluRowOrder { bool built = false; std::vector<int> rank; int depth = 0; int* d_rank = nullptr; };
	IluRowOrder ilu_orders[3];
	double *ilu_dinv2 = nullptr;             ///< [ncell][16]: the factor sweeps' second buffer
	double *ilu_p = nullptr, *ilu_q = nullptr;   ///< [ncell][4]: the solve sweeps' iterates besides the output
	const IluRowOrder& ensureIluOrder(int order);
	/// the pivots of the sweep-based ILU(0) in row order `order`: dinv = (Dt^b)^-1 after b = `build` synchronous
	/// sweeps from Dt^0 = A_ii (b = 0: the SGS pivots), the iterates alternating between dinv and ilu_dinv2 so
	/// that the last lands in dinv
	void iluSweepFactor(int order, int build, const double* diag, const double* lower, const double* upper, double* dinv);

	/// lines of the line-implicit preconditioner (fvhip_implicit_config::prec_lines), built on first use
	/// from the mesh (precond_setup.hpp buildLines)
	LineSet lines{};
	double lines_thr = -1.0;
	std::vector<int> h_line_start, h_line_cells, h_line_faces;   ///< the lines in line order (fvhip_lines)
	void ensureLines(double thr);

	/// aggregation multigrid hierarchy (fvhip_implicit_config::prec_amg), built on first use from the mesh
	/// (precond_setup.hpp amgFineGraph, amgCoarsen); coarsening stops at `levels` levels or when a level has
	/// fewer than 64 rows or shrinks by less than 1.25
	std::vector<AmgLevel> amg;
	int amg_levels = 0;
	double amg_thr = -1.0;
	void ensureAmg(int levels, double thr);
	/// the block smoother's (block, colour) offsets of level C for blocks of R rows, on the device; built and
	/// uploaded when R is first used on the level
	const int* amgBlocks(AmgLevel& C, int R);
	/// Galerkin operators of every coarse level from the finest blocks, and their diagonal inverses
	void amgSetup(const double* diag, const double* lower, const double* upper);

	/// frees one device array of `owned` before the handle's destruction
	void release(const void* p);

	/// fp32 copies of the preconditioner blocks (fvhip_implicit_config::prec_single)
	void ensureSinglePrecond();

	/// MatrixFreeSpatialJacobian::apply on device vectors (internal order), single domain, with |x| from
	/// launch_mf_norm on scratch of its own (the operator over a system is matfreeApply, system.hpp)
	void matfree(const double* x, double* y);
};

#endif
