// hnsw_search_variants.hip -- instantiations of hnsw_search_kernel (hnsw_device.hip.h) for ONE
// (metric, accept rule, row format) triple; build.py compiles this file once per triple
// (-DHNSW_V_METRIC= -DHNSW_V_SEMF= -DHNSW_V_FULL=), in parallel.  Each object exports a launcher and an
// occupancy query over the (NCH, NSLOT) grid; hnsw_capi.hip picks the object by the triple.
// The triple is a compile-time parameter of the kernel because the register allocation of a kernel is
// that of its worst path: with both accept rules and both row shapes in one kernel the d = 128 Ohnsw
// variant needed 88 VGPRs (5 waves/SIMD); on its own it needs 64 (8 waves/SIMD).
#include "hnsw_internal.h"

#ifndef HNSW_V_METRIC
#error "compile with -DHNSW_V_METRIC=0|1 -DHNSW_V_SEMF=0|1 -DHNSW_V_FULL=0|1|2|3|4 (rows: ragged fp32, full fp32, bytes, split fp32, half)"
#endif

using hnsw_dev::IndexView;
using hnsw_dev::SearchArgs;

namespace {

constexpr int M_ = HNSW_V_METRIC, S_ = HNSW_V_SEMF;
constexpr int F_ = HNSW_V_FULL;
// the compact rows (bytes, halves) take rows_in_flight's other column
constexpr bool COMPACT_ = F_ == 2 || F_ == 4;

template <int NCH, int RB, int NSLOT>
hipError_t launch_one(const IndexView &iv, const SearchArgs &a, hipStream_t st) {
    const size_t lds = hnsw_dev::search_lds_words(a.vt_bits, a.blk_bits) * sizeof(uint32_t) + (size_t)a.lds_pad;
    // Visited as bitmap blocks (a.blk_bits > 0; W in three or more registers only) is a kernel of its own: the tag-cache kernels
    // keep their registers
    if constexpr (NSLOT >= 3) {
        if (a.blk_bits > 0 && iv.lcode0 && iv.lcode) {
            hipLaunchKernelGGL((hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, M_, S_, F_, 1>), dim3((unsigned)a.nq), dim3(64), lds, st, iv, a);
            return hipGetLastError();
        }
    }
    SearchArgs b = a;
    b.blk_bits = 0;
    hipLaunchKernelGGL((hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, M_, S_, F_>), dim3((unsigned)a.nq),
                       dim3(64), lds, st, iv, b);
    return hipGetLastError();
}
template <int NCH, int RB, int NSLOT>
int occupancy_one(size_t lds, int blk) {
    int nb = 0;
    hipError_t e;
    if constexpr (NSLOT >= 3) {
        e = blk ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, M_, S_, F_, 1>, 64, lds)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, M_, S_, F_>, 64, lds);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hnsw_dev::hnsw_search_kernel<NCH, RB, NSLOT, M_, S_, F_>, 64, lds);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); nb = 0; }
    return nb;
}

// f(Int<NCH>, Int<RB>, Int<NSLOT>) for this unit's kernel of the shape (nch, nslot)
template <class F> auto with_shape(int nch, int nslot, F &&f) {
    return hnsw_host::with_nch(nch, [&](auto NCH) {
        return hnsw_host::with_nslot_knn<NCH>(nslot, [&](auto NSLOT) { return f(NCH, hnsw_host::Int<hnsw_host::rows_in_flight(NCH, COMPACT_)>{}, NSLOT); });
    });
}

} // namespace

#define HNSW_V_CAT2(a, b, c, d) a##b##_##c##_##d
#define HNSW_V_CAT(a, b, c, d) HNSW_V_CAT2(a, b, c, d)

namespace hnsw_host {

hipError_t HNSW_V_CAT(search_launch_, HNSW_V_METRIC, HNSW_V_SEMF, HNSW_V_FULL)(int nch, int nslot, const IndexView &iv, const SearchArgs &a, hipStream_t st) {
    return with_shape(nch, nslot, [&](auto NCH, auto RB, auto NSLOT) { return launch_one<NCH, RB, NSLOT>(iv, a, st); });
}
int HNSW_V_CAT(search_occupancy_, HNSW_V_METRIC, HNSW_V_SEMF, HNSW_V_FULL)(int nch, int nslot, size_t lds, int blk) {
    return with_shape(nch, nslot, [&](auto NCH, auto RB, auto NSLOT) { return occupancy_one<NCH, RB, NSLOT>(lds, blk); });
}

} // namespace hnsw_host
