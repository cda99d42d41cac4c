// hnsw_bits_asym_walk.hip -- the knn kernel's ROWS = 7 instances (hnsw_device.hip.h: hop_round): the walk over the 1-bit codes of
// option "bit_rows" (hnsw_rows_bits.hip) against a 4-BIT query (option "bit_query_bits" 4), for ONE accept rule; build.py compiles
// this file once per rule (-DHNSW_V_SEMF=0|1).  A twin of hnsw_bits_walk.hip -- the same rows, loads, (NW, NSLOT) grid, batches in
// flight, tags / bitmap-blocks choice -- with one difference: the query is four bit planes of its codes in -7..7, a step is four
// `and` + popcount pairs instead of one `xor` + popcount, and the key is that of the INNER PRODUCT <v, s> with the +-1 vector s the
// row's bits stand for (METRIC 1 whatever the index's metric: for a fixed query, -<y, s> orders the rows as |y - c s| does).  The
// C++ hop loop throughout: no hand-scheduled loop knows the format (HopLoop<..., 7, ...>::available is false).
#include "hnsw_internal.h"

#ifndef HNSW_V_SEMF
#error "compile with -DHNSW_V_SEMF=0|1"
#endif

using hnsw_dev::IndexView;
using hnsw_dev::SearchArgs;

namespace {

constexpr int S_ = HNSW_V_SEMF;

template <int NCH, int RB, int NSLOT>
hipError_t launch_one(const IndexView &iv, const SearchArgs &a, hipStream_t st) {
    const size_t lds = hnsw_dev::search_lds_words(a.vt_bits, a.blk_bits) * sizeof(uint32_t) + (size_t)a.lds_pad;
    if constexpr (NSLOT >= 3) {      // Visited as bitmap blocks: a kernel of its own, as for every row format
        if (a.blk_bits > 0 && iv.lcode0 && iv.lcode) {
            hipLaunchKernelGGL((hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 1, S_, 7, 1>), dim3((unsigned)a.nq), dim3(64), lds, st, iv, a);
            return hipGetLastError();
        }
    }
    SearchArgs b = a;
    b.blk_bits = 0;
    hipLaunchKernelGGL((hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 1, S_, 7>), dim3((unsigned)a.nq), dim3(64), lds, st, iv, b);
    return hipGetLastError();
}
template <int NCH, int RB, int NSLOT>
int occupancy_one(size_t lds, int blk) {
    int nb = 0;
    hipError_t e;
    if constexpr (NSLOT >= 3) {
        e = blk ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 1, S_, 7, 1>, 64, lds)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 1, S_, 7>, 64, lds);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 1, S_, 7>, 64, lds);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); nb = 0; }
    return nb;
}

// f(Int<NW>, Int<RB>, Int<NSLOT>) for this unit's kernel of the shape (nw, nslot): exactly the grid of hnsw_bits_walk.hip
template <class F> auto with_shape(int nw, int nslot, F &&f) {
    auto at = [&](auto NW) {
        return hnsw_host::with_nslot_knn<NW>(nslot, [&](auto NSLOT) { return f(NW, hnsw_host::Int<hnsw_host::rows_in_flight_bits(NW)>{}, NSLOT); });
    };
    return nw == 2 ? at(hnsw_host::Int<2>{}) : at(hnsw_host::Int<1>{});
}

} // namespace

#define HNSW_B_CAT2(a, b) a##b
#define HNSW_B_CAT(a, b) HNSW_B_CAT2(a, b)

namespace hnsw_host {

hipError_t HNSW_B_CAT(search_launch_bits_asym_, HNSW_V_SEMF)(int nch, int nslot, const IndexView &iv, const SearchArgs &a, hipStream_t st) {
    return with_shape(nch, nslot, [&](auto NCH, auto RB, auto NSLOT) { return launch_one<NCH, RB, NSLOT>(iv, a, st); });
}
int HNSW_B_CAT(search_occupancy_bits_asym_, HNSW_V_SEMF)(int nch, int nslot, size_t lds, int blk) {
    return with_shape(nch, nslot, [&](auto NCH, auto RB, auto NSLOT) { return occupancy_one<NCH, RB, NSLOT>(lds, blk); });
}

} // namespace hnsw_host
