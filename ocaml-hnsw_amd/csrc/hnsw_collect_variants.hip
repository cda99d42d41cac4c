// hnsw_collect_variants.hip -- instantiations of hnsw_search_collect_kernel (hnsw_device.hip.h; option "filter_collect") for ONE
// (metric, accept rule, row format) triple; build.py compiles this file once per triple of COLLECT_VARIANTS
// (-DHNSW_V_METRIC= -DHNSW_V_SEMF= -DHNSW_V_FULL=), in parallel, as it does hnsw_search_variants.hip.  Each object exports a
// launcher over the (NCH, NSLOT) grid of the knn kernel; hnsw_capi.hip picks the object by the triple.  Row formats 0 .. 3 only:
// the option needs walk distances that are exact over X.
#include "hnsw_internal.h"

#ifndef HNSW_V_METRIC
#error "compile with -DHNSW_V_METRIC=0|1 -DHNSW_V_SEMF=0|1 -DHNSW_V_FULL=0|1|2|3 (rows: ragged fp32, full fp32, bytes, split fp32)"
#endif

using hnsw_dev::CollectArgs;
using hnsw_dev::IndexView;
using hnsw_dev::SearchArgs;

namespace {

constexpr int M_ = HNSW_V_METRIC, S_ = HNSW_V_SEMF;
constexpr int F_ = HNSW_V_FULL;
static_assert(F_ >= 0 && F_ <= 3, "the collect kernel reads exact rows only");
constexpr bool COMPACT_ = F_ == 2;

template <int NCH, int RB, int NSLOT>
hipError_t launch_one(const IndexView &iv, const SearchArgs &a, const CollectArgs &c, hipStream_t st) {
    // the tag-cache Visited whatever the handle chose for the plain kernel
    SearchArgs b = a;
    b.blk_bits = 0;
    const size_t lds = hnsw_dev::wave_lds_words(b.vt_bits) * sizeof(uint32_t) + (size_t)b.lds_pad;
    hipLaunchKernelGGL((hnsw_dev::hnsw_search_collect_kernel<NCH, RB, NSLOT, M_, S_, F_>), dim3((unsigned)a.nq), dim3(64), lds, st, iv, b, c);
    return hipGetLastError();
}

} // namespace

#define HNSW_V_CAT2(a, b, c, d) a##b##_##c##_##d
#define HNSW_V_CAT(a, b, c, d) HNSW_V_CAT2(a, b, c, d)

namespace hnsw_host {

hipError_t HNSW_V_CAT(collect_launch_, HNSW_V_METRIC, HNSW_V_SEMF, HNSW_V_FULL)(int nch, int nslot, const IndexView &iv, const SearchArgs &a,
                                                                                const CollectArgs &c, hipStream_t st) {
    return with_nch(nch, [&](auto NCH) {
        return with_nslot_knn<NCH>(nslot, [&](auto NSLOT) { return launch_one<NCH, rows_in_flight(NCH, COMPACT_), NSLOT>(iv, a, c, st); });
    });
}

} // namespace hnsw_host
