/** \file krylov.hip
 * \brief Device vector kernels of the Krylov method and the Newton update around it (declarations in
 *   krylov.hpp): the multi-dot, which reads w once per group of KRY_GROUP basis vectors, the multi-AXPYs, the
 *   matrix-free operator's norm, perturbation and combination, the energy norm and the relaxed update. Every
 *   reduction uses a fixed grid and the fixed tree of reduce.hpp, so every GMRES coefficient is reproducible.
 */
#include "krylov.hpp"
#include "blk4.hpp"      // nblk
#include "reduce.hpp"

namespace fvhip {

// Three partitions, kept apart on purpose (system.hpp): a sum's bits depend on its partition
constexpr int KRY_DOT_BLOCKS = 2048;   ///< partial sums per GMRES dot product (8 blocks per CU: enough loads in flight)
constexpr int KRY_GROUP = 8;      ///< dot products per block row of the multi-dot (w read once per 8 basis vectors)
constexpr int KRY_MF_BLOCKS = 1024;    ///< partial sums of the single-domain matrix-free norm (launch_mf_norm)

// -------------------------------------------------------------------------------------------------
// reductions and vector updates
// -------------------------------------------------------------------------------------------------
/// block row y of the grid: products j0 = KRY_GROUP*y .. j0+KRY_GROUP-1 (j == k is w . w)
__global__ __launch_bounds__(256)
void k_mdot_partial(long long n, int k, int kt, const double* __restrict__ V, long long ld,
                    const double* __restrict__ w, double* __restrict__ part)
{
	const int j0 = KRY_GROUP*static_cast<int>(blockIdx.y);
	const double* vp[KRY_GROUP];
	#pragma unroll
	for(int q = 0; q < KRY_GROUP; q++) vp[q] = (j0 + q < k) ? V + static_cast<long long>(j0 + q)*ld : w;
	double acc[KRY_GROUP];
	#pragma unroll
	for(int q = 0; q < KRY_GROUP; q++) acc[q] = 0.0;
	// 16-byte loads (n is a multiple of 4: four unknowns per cell); the same fixed order every call
	const long long n2 = n >> 1;
	const double2* w2 = reinterpret_cast<const double2*>(w);
	for(long long i = blockIdx.x*256LL + threadIdx.x; i < n2; i += 256LL*gridDim.x) {
		const double2 wi = w2[i];
		#pragma unroll
		for(int q = 0; q < KRY_GROUP; q++)
			if(j0 + q < kt) {
				const double2 vi = reinterpret_cast<const double2*>(vp[q])[i];
				acc[q] += vi.x*wi.x;
				acc[q] += vi.y*wi.y;
			}
	}
	block_sum<KRY_GROUP>(acc, part + static_cast<size_t>(j0)*KRY_DOT_BLOCKS + blockIdx.x, KRY_DOT_BLOCKS);
}

/// out[b] = sum of the np partials of product b (one block per product)
__global__ __launch_bounds__(256)
void k_sum_partials(int np, const double* __restrict__ part, double* __restrict__ out)
{
	const double* p = part + static_cast<size_t>(blockIdx.x)*np;
	double acc[1] = {0.0};
	for(int i = threadIdx.x; i < np; i += 256) acc[0] += p[i];
	block_sum<1>(acc, out + blockIdx.x, 1);
}

/// s += c[j] * X[j*ld + i] over j = 0 .. k-1 in order (X read as T rows: double or double2)
template <typename T, typename F>
__device__ __forceinline__ void basis_sum(int k, const double* __restrict__ c, const double* __restrict__ V, long long ld,
                                          long long i, F&& add)
{
	for(int j = 0; j < k; j++) add(c[j], reinterpret_cast<const T*>(V + j*ld)[i]);
}

__global__ __launch_bounds__(256)
void k_maxpy(long long n, int k, const double* __restrict__ V, long long ld, const double* __restrict__ h,
             double* __restrict__ w)
{
	const long long i = blockIdx.x*256LL + threadIdx.x;
	if(i >= n) return;
	double s = 0.0;
	basis_sum<double>(k, h, V, ld, i, [&](double c, double v) { s += c*v; });
	w[i] -= s;
}

/// w -= V h over k basis vectors (k_maxpy's sum, in its order: the same w bit for bit) and |w|^2 of the result,
/// over the multi-dot's fixed partition and tree: the Arnoldi step's new norm without another pass over w
__global__ __launch_bounds__(256)
void k_maxpy_norm(long long n, int k, const double* __restrict__ V, long long ld, const double* __restrict__ h,
                  double* __restrict__ w, double* __restrict__ part)
{
	double acc[1] = {0.0};
	const long long n2 = n >> 1;
	double2* w2 = reinterpret_cast<double2*>(w);
	for(long long i = blockIdx.x*256LL + threadIdx.x; i < n2; i += 256LL*gridDim.x) {
		double sx = 0.0, sy = 0.0;
		basis_sum<double2>(k, h, V, ld, i, [&](double c, double2 v) { sx += c*v.x; sy += c*v.y; });
		double2 wi = w2[i];
		wi.x -= sx; wi.y -= sy;
		w2[i] = wi;
		acc[0] += wi.x*wi.x;
		acc[0] += wi.y*wi.y;
	}
	block_sum<1>(acc, part + blockIdx.x, 1);
}

__global__ __launch_bounds__(256)
void k_lincomb(long long n, int k, const double* __restrict__ V, long long ld, const double* __restrict__ c,
               double* __restrict__ out)
{
	const long long i = blockIdx.x*256LL + threadIdx.x;
	if(i >= n) return;
	double s = 0.0;
	basis_sum<double>(k, c, V, ld, i, [&](double cj, double v) { s += cj*v; });
	out[i] = s;
}

__global__ __launch_bounds__(256)
void k_axpby(long long n, double a, const double* __restrict__ x, double b, double* __restrict__ y)
{
	const long long i = blockIdx.x*256LL + threadIdx.x;
	if(i >= n) return;
	y[i] = b == 0.0 ? a*x[i] : a*x[i] + b*y[i];
}

__global__ void k_pertmag(const double* __restrict__ sq, double eps, double* __restrict__ pm)
{
	if(threadIdx.x == 0 && blockIdx.x == 0) {
		const double xnorm = sqrt(sq[0]);
		pm[0] = xnorm;
		pm[1] = eps/xnorm;
	}
}

__global__ __launch_bounds__(256)
void k_energy_partial(int n, const double* __restrict__ r, const double* __restrict__ area, double* __restrict__ part)
{
	double acc[1] = {0.0};
	for(int e = blockIdx.x*256 + threadIdx.x; e < n; e += 256*gridDim.x)
		acc[0] += r[4*static_cast<size_t>(e)+3]*r[4*static_cast<size_t>(e)+3]*area[e];
	block_sum<1>(acc, part + blockIdx.x, 1);
}

__global__ __launch_bounds__(256)
void k_relaxed_update(int n, gd::Gas G, double minfactor, const double* __restrict__ du, double* __restrict__ u)
{
	const int c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= n) return;
	const double4 a = reinterpret_cast<const double4*>(u)[c];
	const double4 d = reinterpret_cast<const double4*>(du)[c];
	const double uu[4] = {a.x, a.y, a.z, a.w}, dd[4] = {d.x, d.y, d.z, d.w};
	const double om = relaxation_factor(G, minfactor, dd, uu);
	reinterpret_cast<double4*>(u)[c] = make_double4(uu[0] + om*dd[0], uu[1] + om*dd[1], uu[2] + om*dd[2],
	                                                uu[3] + om*dd[3]);
}

// -------------------------------------------------------------------------------------------------
// matrix-free pieces of the single-domain operator (fvhip_ctx::matfree)
// -------------------------------------------------------------------------------------------------
/// deterministic two-stage sum of squares: fixed partition, fixed tree
__global__ __launch_bounds__(256)
void k_sumsq_partial(long long n, const double* __restrict__ x, double* __restrict__ part)
{
	double acc[1] = {0.0};
	for(long long i = blockIdx.x*256LL + threadIdx.x; i < n; i += 256LL*gridDim.x) acc[0] += x[i]*x[i];
	block_sum<1>(acc, part + blockIdx.x, 1);
}

/// out[0] = sqrt(sum(part)), out[1] = eps/out[0]: k_pertmag from the np partial sums of one domain
__global__ __launch_bounds__(256)
void k_mf_pertmag(int np, const double* __restrict__ part, double eps, double* __restrict__ out)
{
	double acc[1] = {0.0};
	for(int i = threadIdx.x; i < np; i += 256) acc[0] += part[i];
	block_sum<1>(acc, out, 1);
	if(threadIdx.x == 0) { out[0] = sqrt(out[0]); out[1] = eps/out[0]; }
}

__global__ __launch_bounds__(256)
void k_mf_perturb(long long n, const double* __restrict__ u, const double* __restrict__ x,
                  const double* __restrict__ pm, double* __restrict__ aux)
{
	const long long i = blockIdx.x*256LL + threadIdx.x;
	if(i >= n) return;
	aux[i] = u[i] + pm[1]*x[i];
}

__global__ __launch_bounds__(256)
void k_mf_combine(int ncell, const double* __restrict__ mdt, const double* __restrict__ x,
                  const double* __restrict__ yg, const double* __restrict__ res,
                  const double* __restrict__ pm, double* __restrict__ y)
{
	const int c = blockIdx.x*256 + threadIdx.x;
	if(c >= ncell) return;
	const double pert = pm[1], d = mdt[c];
	// one 32-byte row per vector and cell; each entry mdt x + (-yg + res)/pert as before
	const double4 xv = reinterpret_cast<const double4*>(x)[c], gv = reinterpret_cast<const double4*>(yg)[c];
	const double4 rv = reinterpret_cast<const double4*>(res)[c];
	reinterpret_cast<double4*>(y)[c] = make_double4(d*xv.x + (-gv.x + rv.x)/pert, d*xv.y + (-gv.y + rv.y)/pert,
	                                                d*xv.z + (-gv.z + rv.z)/pert, d*xv.w + (-gv.w + rv.w)/pert);
}

// -------------------------------------------------------------------------------------------------
// launchers
// -------------------------------------------------------------------------------------------------
void launch_sum_partials(int nproducts, int np, const double* part, double* out, hipStream_t s)
{ k_sum_partials<<<nproducts, 256, 0, s>>>(np, part, out); }

size_t kry_scratch(int k)
{
	return static_cast<size_t>(KRY_DOT_BLOCKS)*static_cast<size_t>((k + KRY_GROUP)/KRY_GROUP*KRY_GROUP);
}

void launch_mdot(long long n, int k, const double* V, long long ld, const double* w, bool self,
                 double* part, double* out, hipStream_t s)
{
	const int kt = k + (self ? 1 : 0);
	if(kt <= 0) return;
	k_mdot_partial<<<dim3(KRY_DOT_BLOCKS, (kt + KRY_GROUP - 1)/KRY_GROUP), 256, 0, s>>>(n, k, kt, V, ld, w, part);
	launch_sum_partials(kt, KRY_DOT_BLOCKS, part, out, s);
}

void launch_maxpy(long long n, int k, const double* V, long long ld, const double* h, double* w, hipStream_t s)
{ if(n > 0 && k > 0) k_maxpy<<<nblk(n,256), 256, 0, s>>>(n, k, V, ld, h, w); }
void launch_maxpy_norm(long long n, int k, const double* V, long long ld, const double* h, double* w, double* part,
                       double* out, hipStream_t s)
{
	k_maxpy_norm<<<KRY_DOT_BLOCKS, 256, 0, s>>>(n, k, V, ld, h, w, part);
	launch_sum_partials(1, KRY_DOT_BLOCKS, part, out, s);
}
void launch_lincomb(long long n, int k, const double* V, long long ld, const double* c, double* out, hipStream_t s)
{ if(n > 0) k_lincomb<<<nblk(n,256), 256, 0, s>>>(n, k, V, ld, c, out); }
void launch_axpby(long long n, double a, const double* x, double b, double* y, hipStream_t s)
{ if(n > 0) k_axpby<<<nblk(n,256), 256, 0, s>>>(n, a, x, b, y); }
void launch_pertmag(const double* sq, double eps, double* pm, hipStream_t s)
{ k_pertmag<<<1, 64, 0, s>>>(sq, eps, pm); }

void launch_energy_sumsq(int n, const double* r, const double* area, double* part, double* out, hipStream_t s)
{
	k_energy_partial<<<RED_CELL_BLOCKS, 256, 0, s>>>(n, r, area, part);
	launch_sum_partials(1, RED_CELL_BLOCKS, part, out, s);
}

void launch_relaxed_update(int n, const gd::Gas& G, double minfactor, const double* du, double* u, hipStream_t s)
{ if(n > 0) k_relaxed_update<<<nblk(n,256), 256, 0, s>>>(n, G, minfactor, du, u); }

void launch_mf_norm(long long n, const double* x, double eps, double* part, double* pm, hipStream_t s)
{
	hipLaunchKernelGGL(k_sumsq_partial, dim3(KRY_MF_BLOCKS), dim3(256), 0, s, n, x, part);
	hipLaunchKernelGGL(k_mf_pertmag, dim3(1), dim3(256), 0, s, KRY_MF_BLOCKS, part, eps, pm);
}

int mf_partials() { return KRY_MF_BLOCKS; }

void launch_mf_perturb(long long n, const double* u, const double* x, const double* pm, double* aux, hipStream_t s)
{
	hipLaunchKernelGGL(k_mf_perturb, dim3(nblk(n,256)), dim3(256), 0, s, n, u, x, pm, aux);
}

void launch_mf_combine(int ncell, const double* mdt, const double* x, const double* yg, const double* res,
                       const double* pm, double* y, hipStream_t s)
{
	hipLaunchKernelGGL(k_mf_combine, dim3(nblk(ncell,256)), dim3(256), 0, s, ncell, mdt, x, yg, res, pm, y);
}

}
