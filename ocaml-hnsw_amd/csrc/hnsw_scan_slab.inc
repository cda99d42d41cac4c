// hnsw_scan_slab.inc -- the body of the exact scan's kernels (hnsw_scan.hip): the scan of one (tile, slab) wave, included once
// per kernel with SCAN_MASKED 0 (hnsw_scan_kernel: every row is a candidate) or 1 (hnsw_scan_masked_kernel: `mask` holds one bit
// per row, bit row & 31 of word row >> 5, ceil(n / 32) words; a row whose bit is clear contributes no candidate, and a 32-row
// word without a set bit is stepped over without loading its rows).  In scope: NCH, METRIC, iv, a.
    constexpr int T = scan_tile(NCH), UB = scan_rows(NCH);
    constexpr bool QLDS = NCH >= 8;
    constexpr int LIMIT = SCAN_BUF - 4 * UB;      // a buffer up to here takes the survivors of one more pass over the UB batches
    __shared__ float4 qs[QLDS ? T * 16 * NCH : 1];
    __shared__ uint64_t bufs[SCAN_WAVES][T][SCAN_BUF];
    __shared__ uint64_t sorted_all[SCAN_WAVES][SCAN_BUF];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane >> 4, l16 = lane & 15;
    const int64_t q0 = (int64_t)blockIdx.x * T;
    const int tq = (int)(a.nq - q0 < T ? a.nq - q0 : T);       // queries of this tile (>= 1: the grid has no empty tile)
    const int k = a.k;

    float4 qv[QLDS ? 1 : T][QLDS ? 1 : NCH];
    if constexpr (QLDS) {       // the workgroup loads the tile once, zero beyond d and beyond the tile's last query
        for (int c = threadIdx.x; c < T * 16 * NCH; c += 64 * SCAN_WAVES) {
            const int t = c / (16 * NCH), e0 = 4 * (c % (16 * NCH));
            const float *qp = a.Q + (q0 + (t < tq ? t : 0)) * a.q_stride;
            float4 v;
            v.x = (t < tq && e0 + 0 < iv.d) ? qp[e0 + 0] : 0.f; v.y = (t < tq && e0 + 1 < iv.d) ? qp[e0 + 1] : 0.f;
            v.z = (t < tq && e0 + 2 < iv.d) ? qp[e0 + 2] : 0.f; v.w = (t < tq && e0 + 3 < iv.d) ? qp[e0 + 3] : 0.f;
            qs[c] = v;
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int t = 0; t < T; ++t) load_query<NCH>(qv[t], a.Q + (q0 + (t < tq ? t : 0)) * a.q_stride, iv.d, l16);
    }
    const int64_t slab = (int64_t)blockIdx.y * SCAN_WAVES + wave;
    if (slab >= a.n_slabs) return;                  // (after the only workgroup barrier)
    const int64_t r0 = slab * a.slab_rows, r1 = r0 + a.slab_rows < iv.n ? r0 + a.slab_rows : iv.n;
    uint64_t *const sorted = sorted_all[wave];

    // per query of the tile: its list's two halves, which half is current (bit t of par), the threshold word, the buffer's fill
    uint64_t *const lists0 = a.lists + ((q0 * a.n_slabs + slab) * 2) * (int64_t)k;
    const int64_t list_step = (int64_t)a.n_slabs * 2 * k;
    uint64_t thr[T];
    int cnt[T];
    uint32_t par = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        // a query past the tile's end never has a survivor (no word is below 0)
        thr[t] = t < tq ? SCAN_EMPTY : 0ull;
        cnt[t] = 0;
        if (t < tq) for (int j = lane; j < k; j += 64) lists0[t * list_step + j] = SCAN_EMPTY;
    }
    scan_wave_sync();

    const uint32_t stride_b = (uint32_t)iv.stride * 4u;
    for (int64_t base = r0; base < r1; base += 4 * UB) {
#if SCAN_MASKED
        if (uniform((int)mask[base >> 5]) == 0) { base = (base | 31) + 1 - 4 * UB; continue; }   // no allowed row in this word: on to the next
#endif
        float4 v[UB][NCH];
#pragma unroll
        for (int u = 0; u < UB; ++u) {              // past the slab's end: its last row again, dropped below
            const int64_t row = base + 4 * u + r;
            const char *rp = reinterpret_cast<const char *>(iv.X) + (uint64_t)(row < r1 ? row : r1 - 1) * stride_b;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = i * 16 + l16;
                v[u][i] = *reinterpret_cast<const float4 *>(rp + 16u * (uint32_t)(c < iv.nchunks ? c : 0));
            }
        }
        bool full = false;
#pragma unroll
        for (int u = 0; u < UB; ++u) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {         // lanes past the row end add exactly 0 (their query chunk is 0)
                const bool cv = (i * 16 + l16) < iv.nchunks;
                v[u][i].x = cv ? v[u][i].x : 0.f; v[u][i].y = cv ? v[u][i].y : 0.f;
                v[u][i].z = cv ? v[u][i].z : 0.f; v[u][i].w = cv ? v[u][i].w : 0.f;
            }
            const int64_t row = base + 4 * u + r;
#if SCAN_MASKED
            const bool allowed = row < r1 && ((mask[row >> 5] >> (row & 31)) & 1u);
#endif
#pragma unroll
            for (int t = 0; t < T; ++t) {
                // (the tile in LDS is read here, every time: left alone the compiler hoists T * NCH float4 reads out of the loops)
                if constexpr (QLDS) asm volatile("" ::: "memory");
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const float4 z = v[u][i];
                    const float4 qi = QLDS ? qs[(t * NCH + i) * 16 + l16] : qv[QLDS ? 0 : t][QLDS ? 0 : i];
                    if (METRIC == 0) {
                        float dx = z.x - qi.x; acc = __builtin_fmaf(dx, dx, acc);
                        float dy = z.y - qi.y; acc = __builtin_fmaf(dy, dy, acc);
                        float dz = z.z - qi.z; acc = __builtin_fmaf(dz, dz, acc);
                        float dw = z.w - qi.w; acc = __builtin_fmaf(dw, dw, acc);
                    } else {
                        acc = __builtin_fmaf(z.x, qi.x, acc);
                        acc = __builtin_fmaf(z.y, qi.y, acc);
                        acc = __builtin_fmaf(z.z, qi.z, acc);
                        acc = __builtin_fmaf(z.w, qi.w, acc);
                    }
                }
                acc = reduce16(acc);
                const uint32_t key = dist_to_key<METRIC>(acc);
                if (ballot(key <= (uint32_t)(thr[t] >> 32))) {           // rare: some row of the four may be among the k smallest
                    const uint64_t e = ((uint64_t)key << 32) | (uint32_t)row;
#if SCAN_MASKED
                    const bool in = l16 == 0 && allowed && e < thr[t];
#else
                    const bool in = l16 == 0 && row < r1 && e < thr[t];
#endif
                    const uint64_t m = ballot(in);
                    if (in) bufs[wave][t][cnt[t] + popc(m & ((1ull << lane) - 1ull))] = e;
                    cnt[t] += popc(m);
                    full = full || cnt[t] > LIMIT;
                }
            }
        }
        if (full) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (cnt[t] > LIMIT) {
                    uint64_t *const A = lists0 + t * list_step;
                    const bool p = (par >> t) & 1u;
                    scan_flush(bufs[wave][t], sorted, cnt[t], A + (p ? k : 0), A + (p ? 0 : k), k, lane);
                    par ^= 1u << t;
                    cnt[t] = 0;
                    thr[t] = scan_uniform64((A + (p ? 0 : k))[k - 1]);
                }
            }
        }
    }
    // what is left in the buffers; the result belongs in the first half
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t >= tq) continue;
        uint64_t *const A = lists0 + t * list_step;
        if (cnt[t] > 0) {
            const bool p = (par >> t) & 1u;
            scan_flush(bufs[wave][t], sorted, cnt[t], A + (p ? k : 0), A + (p ? 0 : k), k, lane);
            par ^= 1u << t;
        }
        if ((par >> t) & 1u) for (int j = lane; j < k; j += 64) A[j] = A[k + j];
    }
