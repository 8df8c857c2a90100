/** \file halo_legs.hpp
 * \brief The legs of a halo exchange between the ranks of one partition held by one process: per rank and
 *   neighbour, where the peer is and which of the peer's neighbour blocks faces back. Layouts only, no device
 *   type, so that the table is checked on the host (tests/native/halo_legs_check.cpp).
 */
#ifndef FVHIP_HALO_LEGS_HPP
#define FVHIP_HALO_LEGS_HPP

#include "layout.hpp"
#include <stdexcept>
#include <vector>

namespace fvhip {

/// rows neighbour k sends / receives in an exchange of `layers` halo layers (a one-layer exchange
/// of a two-layer halo moves the leading layer-1 part of each block)
inline int sendCount(const Layout& L, size_t k, int layers) {
	return (layers >= 2 || L.send_l1_end.empty() ? L.send_start[k+1] : L.send_l1_end[k]) - L.send_start[k];
}
inline int ghostCount(const Layout& L, size_t k, int layers) {
	return (layers >= 2 || L.ghost_l1_end.empty() ? L.ghost_start[k+1] : L.ghost_l1_end[k]) - L.ghost_start[k];
}

/// rank i's neighbour k receives from list entry `peer`, whose neighbour block kk is rank i
struct HaloLeg { int peer, kk; };

struct HaloLegs
{
	std::vector<std::vector<HaloLeg>> of;    ///< [list entry][neighbour k]
	bool any = false;                        ///< some rank has a neighbour
};

/// the legs of the ranks `rank[i]` with layouts `L[i]` (one entry per rank of the partition, in any order);
/// every leg's ghost block has the size of the peer's send block, in a one- and in a two-layer exchange
inline HaloLegs haloLegs(const std::vector<const Layout*>& L, const std::vector<int>& rank)
{
	const int n = static_cast<int>(L.size());
	std::vector<int> byrank(n, -1);
	for(int i = 0; i < n; i++) {
		if(rank[i] < 0 || rank[i] >= n) throw std::logic_error("group: ranks are not 0..n-1");
		byrank[rank[i]] = i;
	}
	HaloLegs T;
	T.of.resize(n);
	for(int i = 0; i < n; i++)
		for(size_t k = 0; k < L[i]->nbr_rank.size(); k++) {
			const int q = L[i]->nbr_rank[k];
			const int p = q >= 0 && q < n ? byrank[q] : -1;
			size_t kk = 0;
			if(p >= 0) while(kk < L[p]->nbr_rank.size() && L[p]->nbr_rank[kk] != rank[i]) kk++;
			if(p < 0 || kk == L[p]->nbr_rank.size()) throw std::logic_error("halo lists are not symmetric");
			for(int layers = 1; layers <= 2; layers++)
				if(ghostCount(*L[i], k, layers) != sendCount(*L[p], kk, layers)) throw std::logic_error("halo sizes differ");
			T.of[i].push_back(HaloLeg{p, static_cast<int>(kk)});
			T.any = true;
		}
	return T;
}

}
#endif
