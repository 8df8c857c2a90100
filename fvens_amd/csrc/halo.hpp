/** \file halo.hpp
 * \brief Device helpers of the ghost-cell exchange (halo.hip).
 */
#ifndef FVHIP_HALO_HPP
#define FVHIP_HALO_HPP

#include <hip/hip_runtime.h>
#include "gasdyn.hpp"

namespace fvhip {

/// dst[i*width + k] = src[idx[i]*width + k] for i < n (rows of owned cells a neighbour needs)
void launch_pack_rows(const int* idx, int n, const double* src, int width, double* dst, hipStream_t s);
/// dst[idx[r]][k] = src[r][k] (the inverse of launch_pack_rows)
void launch_unpack_rows(const int* idx, int n, const double* src, int width, double* dst, hipStream_t s);
/// k_ghost_gather, the exchange of a periodic handle: dst[first + g][0..width) = src[from[g]][0..width) for g < n,
/// in one launch (src and dst may be the same array: rows from[g] lie outside [first, first + n))
void launch_ghost_gather(const int* from, int n, const double* src, int width, double* dst, long long first, hipStream_t s);
/// primitive state of rows [first, first+count) (ghost cells), same arithmetic as k_prep_cells
void launch_cons2prim_rows(const gd::Gas& G, const double* u, double* up, int first, int count, hipStream_t s);

}
#endif
