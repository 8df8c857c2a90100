/** \file linop.hpp
 * \brief One global system (a handle, or all ranks of a partition driven from one process) and the linear
 *   operator and preconditioner of an implicit step on it: the operator and GMRES are in implicit.cpp, the
 *   preconditioner in precond.cpp.
 */
#ifndef FVHIP_LINOP_HPP
#define FVHIP_LINOP_HPP

#include "ctx.hpp"
#include "precond_options.hpp"

#include <vector>

namespace fvhip_detail {

struct System
{
	std::vector<fvhip_ctx*> hs;
	fvhip_ctx::GroupExchange exg;        ///< in-process halo transport of a group, else empty

	size_t size() const { return hs.size(); }
	bool halo() const { return hs[0]->halo(); }
	template <typename F> void each(F&& f) {
		for(size_t i = 0; i < hs.size(); i++) { HC(hipSetDevice(hs[i]->device)); f(i, hs[i]); }
	}
	void exchange(const fvhip_ctx::ArrayOf& arr, int width) {
		if(!halo()) return;
		if(exg) { exg(arr, width, 1); return; }
		each([&](size_t i, fvhip_ctx* h) { h->exchange_rccl(arr(i), width); });
	}
	/// the steppers' residual: every handle's d_r = 0 + (-r(us)) with its local time steps in d_dtm; fills the
	/// ghost rows of us
	void residual(const std::vector<double*>& us) {
		std::vector<const double*> cu(us.begin(), us.end());
		std::vector<double*> rs, dts;
		for(fvhip_ctx* h : hs) { rs.push_back(h->d_r); dts.push_back(h->d_dtm); }
		fvhip_ctx::residual_seq(hs, cu, rs, true, dts, true, exg);
	}
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
	return System{{h}, {}};
}

inline System ofGroup(fvhip_group_s* g) { return System{g->hs, groupExchange(g)}; }

typedef fvhip_ctx::ArrayOf ArrayOf;

/// MatrixFreeSpatialJacobian::apply (alinalg.cpp:142-233) over a system (implicit.cpp)
/// have_norm: |x|^2 is already in iw.red (the line solve that produced x summed it, LinOp::precondition)
void matfreeApply(System& S, const ArrayOf& x, const ArrayOf& y, bool have_norm = false);

/// `sweeps` smoothing sweeps on level C's A_C x = b from the iterate in x (taken as 0 if `zero`). direction: 0
/// forward, 1 backward, 2 alternating from forward. smoother 0: colour Gauss-Seidel over the whole level; 1: inside
/// row blocks of `rows` rows, block-Jacobi between them -- then x is C.x or an array outside the level (copied in
/// and out), and C.x and C.x2 may have traded places afterwards (the result is in what C.x names then). precond.cpp
void smoothLevel(fvhip_ctx* h, fvhip::AmgLevel& C, int smoother, int rows, const double* b, double* x, int sweeps,
                 int direction, bool zero);

/// The linear operator and preconditioner of one implicit step
struct LinOp
{
	System& S;
	fvhip::PrecondOptions o;
	std::vector<const double*> D, Lo, Up;     ///< per handle: diagonal / lower / upper blocks
	const ArrayOf aux = [this](size_t i) { return S.hs[i]->iw.aux; };   ///< each handle's scratch vectors
	const ArrayOf t = [this](size_t i) { return S.hs[i]->iw.t; };

	/// the preconditioner's blocks of handle i in the precision it applies them in (prec_single: the fp32
	/// copies setup() made): f(PrecBlocks); the launch_* overloads select on the pointer type
	template <typename T> struct PrecBlocks { const T *diag, *dinv, *lo, *up; };
	template <typename F> void withBlocks(size_t i, F&& f) {
		const fvhip_ctx::ImplicitWork& w = S.hs[i]->iw;
		if(o.single) f(PrecBlocks<float>{w.sdiag, w.sdinv, w.slo, w.sup});
		else f(PrecBlocks<double>{D[i], w.dinv, Lo[i], Up[i]});
	}

	// the operator (implicit.cpp)
	/// y = A x with the assembled blocks; x has ghost rows, which are filled here
	void blocks(const ArrayOf& x, const ArrayOf& y);
	/// set by a precondition call asked for the norm of its output (the Arnoldi step's z), consumed by the
	/// next apply: the matrix-free operator needs |z| and the line solve summed it while writing z
	bool znorm = false;
	void apply(const ArrayOf& x, const ArrayOf& y);

	// the preconditioner (precond.cpp)
	/// the preconditioner of the current blocks: the line factorisation or the (ILU) diagonal inverses -- with
	/// the multigrid, its finest smoother -- their fp32 copies, and the multigrid's coarse operators.
	/// (PrecondOptions::check refuses prec_lines with prec_gs / prec_ilu, and the multigrid with either.)
	void setup();
	/// z = M^-1 v (z has ghost rows)
	void precondition(const ArrayOf& v, const ArrayOf& z, bool want_norm = false);
	void sweepColour(size_t i, int col, const double* v, double* z);
	void gaussSeidel(const ArrayOf& v, const ArrayOf& z), iluApply(const ArrayOf& v, const ArrayOf& z);
	void iluSweepApply(const ArrayOf& v, const ArrayOf& z), iluSweeps(const ArrayOf& v, const ArrayOf& z);
	void lineSweeps(const ArrayOf& v, const ArrayOf& z, bool want_norm), amgApply(const ArrayOf& v, const ArrayOf& z);
	void smooth0(fvhip_ctx* h, size_t i, const double* v, double* z);
	void residual0(const ArrayOf& v, const ArrayOf& z, const ArrayOf& t);
	void cycle(fvhip_ctx* h, size_t l);
};

struct GmresOut { int iters; double rnorm0, rnorm; };

}
#endif
