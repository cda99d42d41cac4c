// hnsw_sq8_dim_walk.hip -- the knn kernel's ROWS = 5 instances (hnsw_device.hip.h: hop_round): the L2 walk over the per-dimension
// 8-bit codes of option "sq8_dim_rows" (hnsw_rows_sq8_dim.hip), for ONE accept rule; build.py compiles this file once per rule
// (-DHNSW_V_SEMF=0|1).  What hnsw_search_variants.hip is for the other row formats -- a launcher and an occupancy query over the
// (NCH, NSLOT) grid -- in a unit of its own: the format has no inner-product walk (that one is the byte-row search with the
// query scaled, ROWS = 2), so it is no (metric, rule, format) triple of that table.  The C++ hop loop throughout: no
// hand-scheduled loop knows the format (HopLoop<..., 5, ...>::available is false).
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
            hipLaunchKernelGGL((hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 5, 1>), dim3((unsigned)a.nq), dim3(64), lds, st, iv, a);
            return hipGetLastError();
        }
    }
    SearchArgs b = a;
    b.blk_bits = 0;
    hipLaunchKernelGGL((hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 5>), dim3((unsigned)a.nq), dim3(64), lds, st, iv, b);
    return hipGetLastError();
}
template <int NCH, int RB, int NSLOT>
int occupancy_one(size_t lds, int blk) {
    int nb = 0;
    hipError_t e;
    if constexpr (NSLOT >= 3) {
        e = blk ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 5, 1>, 64, lds)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 5>, 64, lds);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 5>, 64, lds);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); nb = 0; }
    return nb;
}

// f(Int<NCH>, Int<RB>, Int<NSLOT>) for this unit's kernel of the shape (nch, nslot)
template <class F> auto with_shape(int nch, int nslot, F &&f) {
    return hnsw_host::with_nch(nch, [&](auto NCH) {
        return hnsw_host::with_nslot_knn<NCH>(nslot, [&](auto NSLOT) { return f(NCH, hnsw_host::Int<hnsw_host::rows_in_flight_sq8_dim(NCH)>{}, NSLOT); });
    });
}

} // namespace

#define HNSW_D_CAT2(a, b) a##b
#define HNSW_D_CAT(a, b) HNSW_D_CAT2(a, b)

namespace hnsw_host {

hipError_t HNSW_D_CAT(search_launch_sq8_dim_, HNSW_V_SEMF)(int nch, int nslot, const IndexView &iv, const SearchArgs &a, hipStream_t st) {
    return with_shape(nch, nslot, [&](auto NCH, auto RB, auto NSLOT) { return launch_one<NCH, RB, NSLOT>(iv, a, st); });
}
int HNSW_D_CAT(search_occupancy_sq8_dim_, HNSW_V_SEMF)(int nch, int nslot, size_t lds, int blk) {
    return with_shape(nch, nslot, [&](auto NCH, auto RB, auto NSLOT) { return occupancy_one<NCH, RB, NSLOT>(lds, blk); });
}

} // namespace hnsw_host
