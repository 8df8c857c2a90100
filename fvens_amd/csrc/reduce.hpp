/** \file reduce.hpp
 * \brief The fixed-tree reduction over a block of 256 threads that every reproducible norm, sum and minimum of
 *   the library goes through (ode.hip, krylov.hip, lines.hip, surface.hip), and the partition of the two-stage
 *   reductions over cells. For .hip files only: the tree holds its operands in LDS.
 */
#ifndef FVHIP_REDUCE_HPP
#define FVHIP_REDUCE_HPP

#include <hip/hip_runtime.h>

namespace fvhip {

/// blocks (partial results) of the two-stage reductions over cells: the energy norm, the conserved sums, the
/// minimum time step. The multi-dot's and the matrix-free norm's partitions are krylov.hip's own
constexpr int RED_CELL_BLOCKS = 512;

/// minimum that propagates NaN (fmin skips it): one NaN time step makes the minimum NaN
__device__ __forceinline__ double nan_min(double a, double b) { return a != a ? a : (b != b ? b : fmin(a, b)); }

struct RedSum { __device__ __forceinline__ double operator()(double a, double b) const { return a + b; } };
struct RedNanMin { __device__ __forceinline__ double operator()(double a, double b) const { return nan_min(a, b); } };

/// fixed-tree reduction over the block (256 threads, every one of them calls) of NV values per thread:
/// s[q][t] = op(s[q][t], s[q][t + w]) for w = 128 .. 1; thread 0 writes out[q*stride]
template <int NV, typename Op>
__device__ __forceinline__ void block_reduce(double (&acc)[NV], double* out, int stride, Op op)
{
	__shared__ double s[NV][256];
	const int t = static_cast<int>(threadIdx.x);
	#pragma unroll
	for(int q = 0; q < NV; q++) s[q][t] = acc[q];
	__syncthreads();
	for(int w = 128; w > 0; w >>= 1) {
		if(t < w) {
			#pragma unroll
			for(int q = 0; q < NV; q++) s[q][t] = op(s[q][t], s[q][t + w]);
		}
		__syncthreads();
	}
	if(t == 0) {
		#pragma unroll
		for(int q = 0; q < NV; q++) out[q*stride] = s[q][0];
	}
}

/// the fixed-tree sum
template <int NV>
__device__ __forceinline__ void block_sum(double (&acc)[NV], double* out, int stride)
{
	block_reduce<NV>(acc, out, stride, RedSum{});
}

/// out[b] = sum of the np partials part[b*np ..] of product b, b < nproducts, by the same tree (k_sum_partials,
/// krylov.hip): the second stage of every two-stage sum
void launch_sum_partials(int nproducts, int np, const double* part, double* out, hipStream_t s);

}
#endif
