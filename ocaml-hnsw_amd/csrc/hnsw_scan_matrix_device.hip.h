// hnsw_scan_matrix_device.hip.h -- what the two kernels that screen float rows with fp32 matrix instructions share (option
// "scan_matrix": the k-scan, hnsw_scan_matrix.hip, and the range scan, hnsw_range_matrix.hip): the accumulator type, the wave's LDS
// ordering and the exact evaluation of a pair the screen could not drop -- the float scan's own arithmetic, so the key is its key.
#pragma once
#include "hnsw_scan_device.hip.h"

namespace hnsw_dev {

typedef float v16f __attribute__((ext_vector_type(16)));

// LDS words one lane wrote, read by the other lanes of its wave: a wave's LDS operations complete in issue order, so the compiler
// alone must be held (scan_wave_sync would also wait for the row loads in flight)
__device__ __forceinline__ void scan_matrix_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The exact key of (row, the query whose chunks lie at qrow in the tile), by one 16-lane group: scan_slab's arithmetic -- lane l16 on
// the chunks l16, l16 + 16, ..., zero beyond the row's end, the fmaf chain, the tree.
template <int NCH, int METRIC>
__device__ __forceinline__ uint32_t scan_matrix_exact_key(const float *rp, int nchunks, const float *qrow, int l16) {
    float4 z[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = i * 16 + l16;
        z[i] = *reinterpret_cast<const float4 *>(rp + 4 * (c < nchunks ? c : 0));
    }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = i * 16 + l16;
        if (c >= nchunks) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc = scan_chain<METRIC>(acc, z[i], *reinterpret_cast<const float4 *>(qrow + 4 * c));
    }
    return dist_to_key<METRIC>(reduce16(acc));
}

} // namespace hnsw_dev
