// hnsw_hop_loop.inc -- one instantiation of the hand-scheduled layer-0 loop: the explicit specialisation
// HopLoop<NCH, NSLOT, METRIC, ROWS, SEM, BLK> (primary template: hnsw_hop_asm.hip.h).  The table hnsw_hop_instances.inc -- which
// says what shapes there are -- includes this file once per shape, with these macros set (they are undefined again at the end):
//   HNSW_LOOP_NSLOT    1, 2, 3, 4, 6 or 8: key registers per lane that hold W (ef <= 64 / 65..128 / 129..192 / 193..256 / 257..384 /
//                      385..512).  Three bodies: one register, two registers, and ONE for three and more whose slot-count dependent
//                      lines are the macro set HNSW_NS(...) = HNSW_NSX_*_<NSLOT> of the generated hnsw_hop_slots.inc
//   HNSW_LOOP_NCH      2 (default): rows of 65..128 dimensions; 4: rows of 129..256 dimensions
//   HNSW_LOOP_BLK      0 (default) Visited is the tag cache; 1 (three or more registers): bitmap blocks over the locality
//                      codes (HNSW_HOP_FILTER_*_BLK): the hop also reads lcode0's row
// and these three, which default to the translation unit's own HNSW_V_FULL / HNSW_V_METRIC / HNSW_V_SEMF (hnsw_search_variants.hip):
//   HNSW_LOOP_ROWS     2: byte rows and a byte-valued query (integer dot products); 1: float32 rows, every chunk of the lane
//                      grid inside the row; 0: float32 rows, ragged (the lanes whose second chunk lies past the row end are
//                      switched off around that chunk's load and arithmetic); 3: split float32 rows (ragged, and the lanes of
//                      the tail chunks read the expanded node's tail row: HNSW_F32_ROW_LOAD_SPLIT)
//   HNSW_LOOP_METRIC   0 L2, 1 inner product
//   HNSW_LOOP_SEM      0 the Ohnsw accept rule; 1 the functor rule: run() returns true when it left a hop in the middle
// What differs between the row formats is the round (ids -> row loads -> sums -> keys -> accept mask: HNSW_HOP_ROUND_* /
// HNSW_F32_ROUND_*) and the per-lane constants in front of the loop; pop, adjacency, visited filter, compaction and
// insertion are the same text.
#ifndef HNSW_LOOP_ROWS
#define HNSW_LOOP_ROWS HNSW_V_FULL
#endif
#ifndef HNSW_LOOP_METRIC
#define HNSW_LOOP_METRIC HNSW_V_METRIC
#endif
#ifndef HNSW_LOOP_SEM
#define HNSW_LOOP_SEM HNSW_V_SEMF
#endif
#ifndef HNSW_LOOP_NCH
#define HNSW_LOOP_NCH 2
#endif
#ifndef HNSW_LOOP_BLK
#define HNSW_LOOP_BLK 0
#endif
#if HNSW_LOOP_BLK && HNSW_LOOP_NSLOT < 3
#error "HNSW_LOOP_BLK: loops with W in three or more registers only"
#endif
// the slot-count dependent parts of the generic body (W in three or more registers): the macro set HNSW_NSX_<WHAT>_<NSLOT> of the
// generated hnsw_hop_slots.inc
#define HNSW_NS_CAT2(a, n) a##n
#define HNSW_NS_CAT(a, n) HNSW_NS_CAT2(a, n)
#define HNSW_NS(what) HNSW_NS_CAT(HNSW_NSX_##what##_, HNSW_LOOP_NSLOT)
// (the block filter uses um0..um3 as scalar scratch: a three-slot loop has three of its own)
#if HNSW_LOOP_BLK && HNSW_LOOP_NSLOT == 3
#define HNSW_LOOP_UM_EXTRA_DECL uint64_t um3;
#define HNSW_LOOP_UM_EXTRA_OUT [um3] "=&s"(um3),
#else
#define HNSW_LOOP_UM_EXTRA_DECL
#define HNSW_LOOP_UM_EXTRA_OUT
#endif
#if HNSW_LOOP_BLK
#define HNSW_X_ADJACENCY HNSW_HOP_ADJACENCY_BLK
#define HNSW_X_ADJACENCY_MISS HNSW_HOP_ADJACENCY_MISS_BLK
#define HNSW_X_FILTER_ISSUE HNSW_HOP_FILTER_ISSUE_BLK
#define HNSW_X_FILTER_COMPACT HNSW_HOP_FILTER_COMPACT_BLK
#define HNSW_X_PREFETCH_LOAD HNSW_HOP_PREFETCH_LOAD_BLK
#define HNSW_X_SETS
#define HNSW_X_DECL uint32_t nc, pnc; const uint64_t lcm = (uint64_t)(uintptr_t)iv.lcode0 - 4ull * (uint64_t)iv.S0; \
    const uint32_t bsm = cx.blk_set_mask, bmb = lds_offset(cx.blk_bm);
#define HNSW_X_OUT [nc] "=&v"(nc), [pnc] "=&v"(pnc),
#define HNSW_X_IN [lcm] "s"(lcm), [bsm] "s"(bsm), [bmb] "s"(bmb),
#if HNSW_LOOP_ROWS == 2
#define HNSW_BLK_REG_0 "%[d0]"
#define HNSW_BLK_REG_1 "%[d1]"
#define HNSW_BLK_REG_2 "%[d2]"
#define HNSW_BLK_REG_3 "%[d3]"
#define HNSW_BLK_REG_4 "%[d4]"
#define HNSW_BLK_REG_5 "%[d5]"
#define HNSW_BLK_REG_6 "%[d6]"
#define HNSW_BLK_REG_7 "%[d7]"
#define HNSW_BLK_REG_8 "%[id0]"
#define HNSW_BLK_REG_9 "%[id1]"
#define HNSW_BLK_REG_10 "%[id2]"
#define HNSW_BLK_REG_11 "%[id3]"
#define HNSW_BLK_REG_12 "%[ta]"
#define HNSW_BLK_REG_13 "%[tb]"
#define HNSW_BLK_REG_14 "%[ckey]"
#define HNSW_BLK_DIR_READ HNSW_BLK_DIR_READ_B8
#define HNSW_BLK_ZERO HNSW_BLK_ZERO_B8
#define HNSW_BLK_CLEAR(AD) HNSW_BLK_CLEAR_B8(AD)
#else
#define HNSW_BLK_REG_0 HNSW_BLK_F32_REG(0)
#define HNSW_BLK_REG_1 HNSW_BLK_F32_REG(1)
#define HNSW_BLK_REG_2 HNSW_BLK_F32_REG(2)
#define HNSW_BLK_REG_3 HNSW_BLK_F32_REG(3)
#define HNSW_BLK_REG_4 HNSW_BLK_F32_REG(4)
#define HNSW_BLK_REG_5 HNSW_BLK_F32_REG(5)
#define HNSW_BLK_REG_6 HNSW_BLK_F32_REG(6)
#define HNSW_BLK_REG_7 HNSW_BLK_F32_REG(7)
#define HNSW_BLK_REG_8 HNSW_BLK_F32_REG(8)
#define HNSW_BLK_REG_9 HNSW_BLK_F32_REG(9)
#define HNSW_BLK_REG_10 HNSW_BLK_F32_REG(10)
#define HNSW_BLK_REG_11 HNSW_BLK_F32_REG(11)
#define HNSW_BLK_REG_12 HNSW_BLK_F32_REG(12)
#define HNSW_BLK_REG_13 HNSW_BLK_F32_REG(13)
#define HNSW_BLK_REG_14 HNSW_BLK_F32_REG(14)
#define HNSW_BLK_DIR_READ HNSW_BLK_DIR_READ_F32
#define HNSW_BLK_ZERO HNSW_BLK_ZERO_F32
#define HNSW_BLK_CLEAR(AD) HNSW_BLK_CLEAR_F32(AD)
#endif
#else
#define HNSW_X_ADJACENCY HNSW_HOP_ADJACENCY
#define HNSW_X_ADJACENCY_MISS HNSW_HOP_ADJACENCY_MISS
#define HNSW_X_FILTER_ISSUE HNSW_HOP_FILTER_ISSUE
#define HNSW_X_FILTER_COMPACT HNSW_HOP_FILTER_COMPACT
#define HNSW_X_PREFETCH_LOAD HNSW_HOP_PREFETCH_LOAD
#define HNSW_X_SETS const uint32_t setm = cx.set_mask, setb = (uint32_t)cx.set_bits;
#define HNSW_X_DECL
#define HNSW_X_OUT
#define HNSW_X_IN [setm] "s"(setm), [setb] "s"(setb), HNSW_LOOP_TSH_OPERAND
#endif
#if (HNSW_LOOP_NSLOT >= 3 || (HNSW_LOOP_NSLOT == 2 && HNSW_LOOP_ROWS != 2)) && !HNSW_LOOP_BLK
#define HNSW_LOOP_VT3 1
#define HNSW_LOOP_TSH_OPERAND [tsh] "s"(cx.tag_shift),
#define HNSW_VT_WAYS_TEST HNSW_VT_RUNTIME_TEST
#define HNSW_VT_WAYS_JOIN HNSW_VT_RUNTIME_JOIN
#define HNSW_VT_SHIFT HNSW_VT_RUNTIME_SHIFT
#define HNSW_VT_WAYS_RARE HNSW_VT_RUNTIME_RARE
#else
#define HNSW_LOOP_VT3 0
#define HNSW_LOOP_TSH_OPERAND
#define HNSW_VT_WAYS_TEST HNSW_VT_TWO_WAYS_TEST
#define HNSW_VT_WAYS_JOIN HNSW_VT_TWO_WAYS_JOIN
#define HNSW_VT_SHIFT HNSW_VT_TWO_WAYS_SHIFT
#define HNSW_VT_WAYS_RARE HNSW_VT_TWO_WAYS_RARE
#endif
#if HNSW_LOOP_ROWS == 3
#define HNSW_SPLIT_HOP HNSW_SPLIT_HOP_ON
#define HNSW_SPLIT_COMPACT HNSW_SPLIT_COMPACT_ON
#else
#define HNSW_SPLIT_HOP
#define HNSW_SPLIT_COMPACT
#endif
#if HNSW_LOOP_SEM == 0
#define HNSW_SEM_ACCEPT "gt"
#define HNSW_SEM_REJECT "18f"
#define HNSW_EVICT_TIE(LBL, BACK, LASTLO, FULL) HNSW_EVICT_TIE_PUSH(LBL, BACK, LASTLO, FULL)
#define HNSW_SEM_RARE
#define HNSW_SEM_INIT
#else
#define HNSW_SEM_ACCEPT "ge"
#define HNSW_SEM_REJECT "17f"
#define HNSW_EVICT_TIE(LBL, BACK, LASTLO, FULL) HNSW_EVICT_TIE_BAIL(LBL, BACK, LASTLO, FULL)
// 17: the candidate is not below max(W): above -> rejected; AT max(W) with W full -> Nearest.insert_distance answers Inserted
// without changing W and the node joins VisitMe (lib/hnsw.ml:501-504, lib/hnsw_algo.ml:360-364): the tie set's business.
// 98: the loop is left in the middle of a round: the candidates not yet dealt with stay in `fresh` (keys and low key halves
// in ckey / cid), cnt and lastad say which rounds remain; search_layer finishes the hop and comes back when the set is empty
#define HNSW_SEM_RARE                                                                    \
    "17:\n\t"                                                                            \
    "s_cmp_lg_u32 %[kd], %[wmax]\n\t"                                                    \
    "s_cbranch_scc1 18b\n\t"                                                             \
    "s_cmp_eq_u32 %[wmax], -2\n\t"                                                       \
    "s_cbranch_scc1 18b\n"                                                               \
    "98:\n\t"                                                                            \
    "s_mov_b32 %[bail], 1\n\t"                                                           \
    "s_branch 99f\n"
#define HNSW_SEM_INIT "s_mov_b32 %[bail], 0\n\t"
#endif
#if HNSW_LOOP_ROWS == 2
#define HNSW_LOOP_CONSTANTS HNSW_HOP_CONSTANTS
#if HNSW_LOOP_NCH == 4
#define HNSW_LOOP_ROUND_COMMON HNSW_HOP_ROUND_COMMON_N4
#define HNSW_LOOP_ROUNDS_RARE HNSW_HOP_ROUNDS_RARE_N4
#define HNSW_LOOP_AFTER_INSERT HNSW_HOP_AFTER_INSERT_PLAIN
#else
#define HNSW_LOOP_ROUND_COMMON HNSW_HOP_ROUND_COMMON
#define HNSW_LOOP_ROUNDS_RARE HNSW_HOP_ROUNDS_RARE
#define HNSW_LOOP_AFTER_INSERT HNSW_HOP_AFTER_INSERT      /* (round pipelining: a second round's loads run under the first round's insertions) */
#endif
#if HNSW_LOOP_METRIC == 0
#define HNSW_B8_DOTS(DA, DB, TA) HNSW_DOTS(DA, DB, TA)
#define HNSW_B8_DOTS_N4(DA, DB, DC, DD, TA) HNSW_DOTS_N4(DA, DB, DC, DD, TA)
#define HNSW_B8_COMBINE(DA, TA) HNSW_COMBINE(DA, TA)
#define HNSW_B8_KEY(SRC) HNSW_B8_KEY_L2(SRC)
#else
#define HNSW_B8_DOTS(DA, DB, TA) HNSW_DOTS_IP(DA, DB, TA)
#define HNSW_B8_DOTS_N4(DA, DB, DC, DD, TA) HNSW_DOTS_IP_N4(DA, DB, DC, DD, TA)
#define HNSW_B8_COMBINE(DA, TA) HNSW_COMBINE_IP(DA, TA)
#define HNSW_B8_KEY(SRC) HNSW_B8_KEY_IP(SRC)
#endif
#else
#define HNSW_LOOP_CONSTANTS HNSW_F32_CONSTANTS
#define HNSW_LOOP_ROUND_COMMON HNSW_F32_ROUND_COMMON
#if HNSW_LOOP_NCH == 4        /* rows of 129..256 dimensions: four chunks per lane, rounds of 4 and 8 rows */
#define HNSW_LOOP_AFTER_INSERT HNSW_HOP_AFTER_INSERT_PLAIN
#define HNSW_LOOP_ROUNDS_RARE HNSW_F32_ROUND_4ROWS
#define HNSW_F32_ROUND_PICK
#define HNSW_F32_VM1B "4"
#define HNSW_FX_BS "16"
#else
#define HNSW_LOOP_AFTER_INSERT HNSW_HOP_AFTER_INSERT         /* (round pipelining, as the byte rows) */
#define HNSW_LOOP_ROUNDS_RARE HNSW_F32_ROUNDS_RARE
#define HNSW_F32_ROUND_PICK HNSW_F32_ROUND_PICK16
#define HNSW_F32_VM1B "2"
#define HNSW_FX_BS "8"
#endif
#if HNSW_LOOP_NCH == 4 && (HNSW_LOOP_ROWS == 0 || HNSW_LOOP_ROWS == 3)
#define HNSW_F32_RAG_ON
#define HNSW_F32_RAG_OFF "s_mov_b64 exec, -1\n\t"
#elif HNSW_LOOP_ROWS == 0 || HNSW_LOOP_ROWS == 3
#define HNSW_F32_RAG_ON "s_mov_b64 exec, %[cvm]\n\t"
#define HNSW_F32_RAG_OFF "s_mov_b64 exec, -1\n\t"
#else
#define HNSW_F32_RAG_ON
#define HNSW_F32_RAG_OFF
#endif
#if HNSW_LOOP_NCH == 4 && (HNSW_LOOP_ROWS == 0 || HNSW_LOOP_ROWS == 3)
#define HNSW_F32_RAG2_ON "s_mov_b64 exec, %[cvm2]\n\t"
#define HNSW_F32_RAG3_ON "s_mov_b64 exec, %[cvm3]\n\t"
#else
#define HNSW_F32_RAG2_ON
#define HNSW_F32_RAG3_ON
#endif
#if HNSW_LOOP_NCH == 4 && HNSW_LOOP_ROWS == 3
#define HNSW_F32_ROW_LOAD(ID, PJ, AD, B) HNSW_F32_ROW_LOAD_N4_SPLIT(ID, PJ, AD, B)
#elif HNSW_LOOP_NCH == 4
#define HNSW_F32_ROW_LOAD(ID, PJ, AD, B) HNSW_F32_ROW_LOAD_N4(ID, PJ, AD, B)
#elif HNSW_LOOP_ROWS == 3
#define HNSW_F32_ROW_LOAD(ID, PJ, AD, B) HNSW_F32_ROW_LOAD_SPLIT(ID, PJ, AD, B)
#else
#define HNSW_F32_ROW_LOAD(ID, PJ, AD, B) HNSW_F32_ROW_LOAD_PLAIN(ID, PJ, AD, B)
#endif
#if HNSW_LOOP_ROWS == 3
#define HNSW_F32_ID_READ0(ID, PJ, SH) HNSW_F32_ID_READ0_SPLIT(ID, PJ, SH)
#define HNSW_F32_ID_READN(ID, PJ) HNSW_F32_ID_READN_SPLIT(ID, PJ)
#define HNSW_F32_LG0 "0"
#define HNSW_F32_LG1 "2"
#define HNSW_F32_LG2 "4"
#define HNSW_F32_LG3 "6"
#else
#define HNSW_F32_ID_READ0(ID, PJ, SH) HNSW_F32_ID_READ0_PLAIN(ID, PJ, SH)
#define HNSW_F32_ID_READN(ID, PJ) HNSW_F32_ID_READN_PLAIN(ID, PJ)
#define HNSW_F32_LG0 "0"
#define HNSW_F32_LG1 "1"
#define HNSW_F32_LG2 "2"
#define HNSW_F32_LG3 "3"
#endif
#if HNSW_LOOP_METRIC == 0
#if HNSW_LOOP_NCH == 4
#define HNSW_F32_DIST(B) HNSW_F32_DIST_L2_N4(B)
#else
#define HNSW_F32_DIST(B) HNSW_F32_DIST_L2(B)
#endif
#define HNSW_F32_SUM "%[ckey]"
#define HNSW_F32_KEY
#else
#if HNSW_LOOP_NCH == 4
#define HNSW_F32_DIST(B) HNSW_F32_DIST_IP_N4(B)
#else
#define HNSW_F32_DIST(B) HNSW_F32_DIST_IP(B)
#endif
#define HNSW_F32_SUM "%[t1]"
#define HNSW_F32_KEY HNSW_F32_KEY_IP
#endif
#endif

// ---- the frame around the three assembler texts, written once: the operand lists.  Their ORDER is part of the program (the register
// allocator takes the constraints in order), so a body's own operands -- W, the um* / mx* / g0 scratch registers, the debug hop
// limit -- are written at its asm statement, between these pieces:
//   HNSW_LOOP_OUT_A    the loop state (wmax .. od), the block filter's registers, the per-lane temporaries up to the row addresses
//   HNSW_LOOP_OUT_B    the scalar temporaries from `fresh` to the saved m0
//   HNSW_LOOP_OUT_BAIL the functor rule's flag, last
//   HNSW_LOOP_IN       the query, the tables and LDS offsets, the row format's constants
#if HNSW_LOOP_ROWS == 2
#define HNSW_LOOP_ROW_OUT [q2v] "=&v"(q2v),
#define HNSW_LOOP_ROW_CLOBBER
#elif HNSW_LOOP_ROWS == 3
#define HNSW_LOOP_ROW_OUT [pj0] "=&v"(pj0), [pj1] "=&v"(pj1), [pj2] "=&v"(pj2), [pj3] "=&v"(pj3), [trow] "=&v"(trow), [hopn] "=&s"(hopn),
#define HNSW_LOOP_ROW_CLOBBER HNSW_F32_CLOBBER HNSW_SPLIT_CLOBBER
#else
#define HNSW_LOOP_ROW_OUT
#define HNSW_LOOP_ROW_CLOBBER HNSW_F32_CLOBBER
#endif
#if HNSW_LOOP_ROWS == 2 && HNSW_LOOP_NCH == 4
#define HNSW_LOOP_D_OUT [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2), [d3] "=&v"(d3), [d4] "=&v"(d4), [d5] "=&v"(d5), [d6] "=&v"(d6), [d7] "=&v"(d7), \
          [d8] "=&v"(d8), [d9] "=&v"(d9), [d10] "=&v"(d10), [d11] "=&v"(d11), [d12] "=&v"(d12), [d13] "=&v"(d13), [d14] "=&v"(d14), [d15] "=&v"(d15),
#elif HNSW_LOOP_ROWS == 2
#define HNSW_LOOP_D_OUT [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2), [d3] "=&v"(d3), [d4] "=&v"(d4), [d5] "=&v"(d5), [d6] "=&v"(d6), [d7] "=&v"(d7),
#else
#define HNSW_LOOP_D_OUT       /* the rows: HNSW_FX registers, by name (HNSW_F32_CLOBBER) */
#endif
#define HNSW_LOOP_OUT_A \
          [wmax] "+&s"(wmax), [nd] "+&s"(nd), [nh] "+&s"(nh), [st] "+&s"(st), [oc] "+&s"(oc), [od] "+&s"(od), \
          HNSW_X_OUT \
          [nb] "=&v"(nb), [pnb] "=&v"(pnb), [vw] "=&v"(vw), [va] "=&v"(va), [tag] "=&v"(tag), [r4] "=&v"(r4), \
          [co] "=&v"(co), HNSW_LOOP_ROW_OUT \
          [id0] "=&v"(id0), [id1] "=&v"(id1), [id2] "=&v"(id2), [id3] "=&v"(id3), \
          HNSW_LOOP_D_OUT \
          [ta] "=&v"(ta), [tb] "=&v"(tb), [ckey] "=&v"(ckey), [cid] "=&v"(cid), [t0] "=&v"(t0), [t1] "=&v"(t1), \
          [ad0] "=&v"(ad0), [ad1] "=&v"(ad1),
#define HNSW_LOOP_OUT_B \
          [fresh] "=&s"(fresh), [b3m] "=&s"(b3m), [b2m] "=&s"(b2m), \
          [pref] "=&s"(pref), [cnt] "=&s"(cnt), \
          [sx] "=&s"(sx), [lastad] "=&s"(lastad), [i] "=&s"(i), [kd] "=&s"(kd), [klo] "=&s"(klo), [p] "=&s"(p), [t] "=&s"(t), \
          [nw] "=&s"(nw), [tmp] "=&s"(tmp), [sm0] "=&s"(sm0)
#if HNSW_LOOP_SEM
#define HNSW_LOOP_OUT_BAIL , [bail] "=&s"(bail)
#else
#define HNSW_LOOP_OUT_BAIL
#endif
#if HNSW_LOOP_ROWS == 2 && HNSW_LOOP_NCH == 4
#define HNSW_LOOP_QUERY_IN [qb0] "v"(cx.qb[0]), [qb1] "v"(cx.qb[1]), [xl] "v"(xl), [lane] "v"(cx.lane), [qb2] "v"(cx.qb[2]), [qb3] "v"(cx.qb[3]),
#elif HNSW_LOOP_ROWS == 2
#define HNSW_LOOP_QUERY_IN [qb0] "v"(cx.qb[0]), [qb1] "v"(cx.qb[1]), [xl] "v"(xl), [lane] "v"(cx.lane),
#elif HNSW_LOOP_NCH == 4
#define HNSW_LOOP_QUERY_IN [qf0] "v"(qv[0].x), [qf1] "v"(qv[0].y), [qf2] "v"(qv[0].z), [qf3] "v"(qv[0].w), \
          [qf4] "v"(qv[1].x), [qf5] "v"(qv[1].y), [qf6] "v"(qv[1].z), [qf7] "v"(qv[1].w), [xl] "v"(xl), [lane] "v"(cx.lane), \
          [qf8] "v"(qv[2].x), [qf9] "v"(qv[2].y), [qf10] "v"(qv[2].z), [qf11] "v"(qv[2].w), \
          [qf12] "v"(qv[3].x), [qf13] "v"(qv[3].y), [qf14] "v"(qv[3].z), [qf15] "v"(qv[3].w),
#else
#define HNSW_LOOP_QUERY_IN [qf0] "v"(qv[0].x), [qf1] "v"(qv[0].y), [qf2] "v"(qv[0].z), [qf3] "v"(qv[0].w), \
          [qf4] "v"(qv[1].x), [qf5] "v"(qv[1].y), [qf6] "v"(qv[1].z), [qf7] "v"(qv[1].w), [xl] "v"(xl), [lane] "v"(cx.lane),
#endif
#if HNSW_LOOP_ROWS == 2
#define HNSW_LOOP_ROW_IN , [q2] "s"(q2)
#elif HNSW_LOOP_ROWS == 1
#define HNSW_LOOP_ROW_IN
#elif HNSW_LOOP_ROWS == 0 && HNSW_LOOP_NCH == 4
#define HNSW_LOOP_ROW_IN , [cvm2] "s"(cvm2), [cvm3] "s"(cvm3)
#elif HNSW_LOOP_ROWS == 0
#define HNSW_LOOP_ROW_IN , [cvm] "s"(cvm)
#elif HNSW_LOOP_NCH == 4
#define HNSW_LOOP_ROW_IN , [cvm2] "s"(cvm2), [cvm3] "s"(cvm3), [tlm2] "s"(tlm2), [tlm3] "s"(tlm3), [c16t] "s"(c16t), [s0tv] "v"(s0tv), [tbase] "v"(tbase)
#else
#define HNSW_LOOP_ROW_IN , [cvm] "s"(cvm), [tlm] "s"(tlm), [c16t] "s"(c16t), [s0tv] "v"(s0tv), [tbase] "v"(tbase)
#endif
#define HNSW_LOOP_IN HNSW_LOOP_QUERY_IN \
          [nbrm] "s"(nbrm), [rowm] "s"(rowm), [rowb] "s"(rowb), [st8] "s"(st8), [vtb] "s"(vtb), HNSW_X_IN \
          [cand] "s"(cand), [candm4] "s"(cand - 4u) HNSW_LOOP_ROW_IN

#if HNSW_LOOP_NSLOT != 1 && HNSW_LOOP_NSLOT != 2 && HNSW_LOOP_NSLOT != 3 && HNSW_LOOP_NSLOT != 4 && HNSW_LOOP_NSLOT != 6 && HNSW_LOOP_NSLOT != 8
#error "HNSW_LOOP_NSLOT: 1, 2, 3, 4, 6 or 8"
#endif
template <> struct HopLoop<HNSW_LOOP_NCH, HNSW_LOOP_NSLOT, HNSW_LOOP_METRIC, HNSW_LOOP_ROWS, HNSW_LOOP_SEM, HNSW_LOOP_BLK> {
    static constexpr bool available = true;
    static __device__ __forceinline__ bool run(const IndexView &iv, WList<HNSW_LOOP_NSLOT> &w, const WaveCtx &cx, HopResume &rs,
                                               const float4 (&qv)[HNSW_LOOP_NCH], uint32_t &n_dist, uint32_t &n_hops, uint32_t &status,
                                               uint32_t maxhops = 0xFFFFFFFFu) {
    (void)rs; (void)qv; (void)maxhops;
#if HNSW_LOOP_ROWS == 2
    const uint64_t xl = (uint64_t)(uintptr_t)iv.X8 + 4u * (uint32_t)cx.l16;
#elif HNSW_LOOP_ROWS == 3
    const uint64_t xl = (uint64_t)(uintptr_t)iv.Xm + 16u * (uint32_t)cx.l16;
#else
    const uint64_t xl = (uint64_t)(uintptr_t)iv.X + 16u * (uint32_t)cx.l16;
#endif
    const uint64_t nbrm = (uint64_t)(uintptr_t)iv.nbr0 - 4ull * (uint64_t)iv.S0;   // one row before the table: rows are addressed by id + 1
    const uint64_t rowm = iv.S0 >= 64 ? ~0ull : ((1ull << iv.S0) - 1ull);
#if HNSW_LOOP_ROWS == 2
    const uint32_t rowb = (uint32_t)iv.S0 * 4u, st8 = (uint32_t)iv.stride8;
#elif HNSW_LOOP_ROWS == 3
    const uint32_t rowb = (uint32_t)iv.S0 * 4u, st8 = (uint32_t)iv.stride_m;      // st8: bytes from one main row to the next
#else
    const uint32_t rowb = (uint32_t)iv.S0 * 4u, st8 = (uint32_t)iv.stride * 4u;   // st8: bytes from one row to the next
#endif
    const uint32_t vtb = lds_offset(cx.vt), cand = lds_offset(cx.cand_id);
    HNSW_X_SETS
#if HNSW_LOOP_NCH == 4 && (HNSW_LOOP_ROWS == 0 || HNSW_LOOP_ROWS == 3)
    const uint64_t cvm2 = ballot(32 + cx.l16 < iv.nchunks), cvm3 = ballot(48 + cx.l16 < iv.nchunks);   // lanes whose third / fourth chunk lies inside the row
#elif HNSW_LOOP_ROWS == 0 || HNSW_LOOP_ROWS == 3
    const uint64_t cvm = ballot(16 + cx.l16 < iv.nchunks);   // lanes whose second chunk lies inside the row
#endif
#if HNSW_LOOP_ROWS == 3 && HNSW_LOOP_NCH == 4
    // split rows of 129..256 dimensions: the tail chunks (the row's last one or two) lie in chunk column 2 or in column 3
    const bool tail2 = 32 + cx.l16 >= iv.main_chunks && 32 + cx.l16 < iv.nchunks, tail3 = 48 + cx.l16 >= iv.main_chunks && 48 + cx.l16 < iv.nchunks;
    const uint64_t tlm2 = ballot(tail2), tlm3 = ballot(tail3);
    const uint32_t c16t = 16u * (uint32_t)iv.tail_chunks, s0tv = (uint32_t)iv.S0 * c16t;
    const uint64_t tbase = (uint64_t)(uintptr_t)iv.tail0 - (uint64_t)s0tv +
                           (tail2 ? 16u * (uint32_t)(32 + cx.l16 - iv.main_chunks) : tail3 ? 16u * (uint32_t)(48 + cx.l16 - iv.main_chunks) : 0u) -
                           (tail2 ? 512ull : 768ull);
    uint32_t pj0, pj1, pj2, pj3, hopn;
    uint64_t trow;
#elif HNSW_LOOP_ROWS == 3
    // split rows: the lanes whose second chunk is one of the tail chunks; their address in the tail row of node (id + 1) - 1 at
    // slot 0, less the 256 the load adds; bytes per tail row and per slot
    const bool tail_lane = 16 + cx.l16 >= iv.main_chunks && 16 + cx.l16 < iv.nchunks;
    const uint64_t tlm = ballot(tail_lane);
    const uint32_t c16t = 16u * (uint32_t)iv.tail_chunks, s0tv = (uint32_t)iv.S0 * c16t;
    const uint64_t tbase = (uint64_t)(uintptr_t)iv.tail0 - (uint64_t)s0tv + (tail_lane ? 16u * (uint32_t)(16 + cx.l16 - iv.main_chunks) : 0u) - 256ull;
    uint32_t pj0, pj1, pj2, pj3, hopn;
    uint64_t trow;
#endif
#if HNSW_LOOP_ROWS == 2
    const uint32_t q2 = (uint32_t)uniform(cx.q2);
#endif
    uint32_t wmax = (uint32_t)uniform((int)w.wmax), nd = (uint32_t)uniform((int)n_dist), nh = (uint32_t)uniform((int)n_hops);
    uint32_t st = (uint32_t)uniform((int)status), oc = (uint32_t)uniform(w.ovf_cnt), od = wmax;   // od: the tie list's distance
    // temporaries
#if HNSW_LOOP_ROWS == 2
    uint32_t nb, pnb, vw, va, tag, r4, co, q2v, id0, id1, id2, id3, d0, d1, d2, d3, d4, d5, d6, d7, ta, tb, ckey, cid, t0, t1;
#if HNSW_LOOP_NCH == 4
    uint32_t d8, d9, d10, d11, d12, d13, d14, d15;      // four dwords per row and batch
#endif
#else
    uint32_t nb, pnb, vw, va, tag, r4, co, id0, id1, id2, id3, ta, tb, ckey, cid, t0, t1;   // the rows: HNSW_FX registers, by name
#endif
    uint64_t ad0, ad1;    // row addresses, alternating by batch (a load has long read its address when the register's next turn comes)
    uint32_t sm0;         // m0 as the block found it
    HNSW_X_DECL
#if HNSW_LOOP_SEM
    uint32_t bail;        // set when the loop is left for the functor rule's tie set (labels 17 / 98)
#endif
#if HNSW_LOOP_NSLOT == 1
    uint64_t um0, um1;    // um1: the visited filter's second compare only
#elif HNSW_LOOP_NSLOT == 2
    uint64_t um0, um1, g0;   // um0 / um1 double as the insertion's equality masks
#else
    HNSW_NS(DECL) HNSW_LOOP_UM_EXTRA_DECL
#endif
    uint64_t fresh, b3m, b2m;   // fresh: the round's accept mask
    uint32_t pref, cnt, sx, lastad, i, kd, klo, p, t, nw, tmp;   // kd doubles as the hop's node (its low key half, id + 1), sx / tmp as the shift's carries
#if HNSW_LOOP_NSLOT == 1        /* ---- the text for W in one key register per lane */
    asm volatile(
        // low key halves inside the loop: id + 1 with the expanded flag in bit 31 (a rotation of the (id + 1) << 1 | flag the
        // rest of the kernel keeps): the unexpanded members are the non-negative ones, a node id is one subtraction away
        "s_mov_b32 %[sm0], m0\n\t"                                       // m0 (lane select of v_writelane) is handed back as it was: not a clobber
        "v_alignbit_b32 %[l0], %[l0], %[l0], 1\n\t"
        HNSW_LOOP_CONSTANTS
        HNSW_SEM_INIT
        "s_mov_b32 %[pref], -1\n"
        HNSW_ASM_ALIGN_K(HNSW_ASM_ALIGN_PAD1)
        "1:\n\t"
        "v_cmp_lt_i32_e64 %[um0], -1, %[l0]\n"
        HNSW_POP_SLOT0("%[um0]", "%[l0]", "90f")
        "3:\n"                                                          // kd = the node's low key half, id + 1
        HNSW_HOP_ADJACENCY
        HNSW_HOP_FILTER_ISSUE
        "s_mov_b32 %[pref], -1\n\t"
        HNSW_PEEK_SLOT0("%[um0]", "%[l0]", "9f")
        HNSW_HOP_PREFETCH_LOAD
        HNSW_HOP_FILTER_COMPACT
        HNSW_LOOP_ROUND_COMMON
        "50:\n\t"
        HNSW_INSERT_LOOP1
        HNSW_LOOP_AFTER_INSERT
        HNSW_HOP_ADJACENCY_MISS
        HNSW_LOOP_ROUNDS_RARE
        HNSW_INSERT_RARE1
        HNSW_VT_WAYS_RARE
        HNSW_SEM_RARE
        HNSW_HOP_TAIL
        // back to the flag-in-bit-0 form
        "\n\ts_mov_b32 m0, %[sm0]"
        "\n\tv_alignbit_b32 %[l0], %[l0], %[l0], 31"
        : [h0] "+&v"(w.hi[0]), [l0] "+&v"(w.lo[0]),
          HNSW_LOOP_OUT_A
          [um0] "=&s"(um0), [um1] "=&s"(um1),
          HNSW_LOOP_OUT_B HNSW_LOOP_OUT_BAIL
        : HNSW_LOOP_IN
        : "vcc", "scc", "memory" HNSW_LOOP_ROW_CLOBBER);
#elif HNSW_LOOP_NSLOT == 2      /* ---- ... in two */
    asm volatile(
        // low key halves inside the loop: id + 1 with the expanded flag in bit 31 (a rotation of the (id + 1) << 1 | flag the
        // rest of the kernel keeps): the unexpanded members are the non-negative ones, a node id is one subtraction away
        "s_mov_b32 %[sm0], m0\n\t"                                       // m0 (lane select of v_writelane) is handed back as it was: not a clobber
        "v_alignbit_b32 %[l0], %[l0], %[l0], 1\n\t"
        "v_alignbit_b32 %[l1], %[l1], %[l1], 1\n\t"
        HNSW_LOOP_CONSTANTS
        HNSW_SEM_INIT
        "s_mov_b32 %[pref], -1\n"
        HNSW_ASM_ALIGN
        // ================================ one hop ================================
        "1:\n\t"
#ifdef HNSW_ASM_DEBUG
        "s_cmp_ge_u32 %[nh], %[maxh]\n\t"                                 // debugging: leave after maxh hops, the C++ loop goes on from here
        "s_cbranch_scc1 99f\n\t"
#endif
        HNSW_PROBE(0)
        // pop: the first unexpanded member of W (pop_min, :565) and its flag; it is nearly always in the lower slot (the
        // upper one: label 2, behind the loop)
        "v_cmp_lt_i32_e64 %[um0], -1, %[l0]\n\t"
        "v_cmp_lt_i32_e64 %[um1], -1, %[l1]\n\t"
        "s_cmp_eq_u64 %[um0], 0\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_ff1_i32_b64 %[i], %[um0]\n\t"
        "v_readlane_b32 %[kd], %[l0], %[i]\n\t"
        "s_bitset0_b64 %[um0], %[i]\n\t"
        "s_mov_b32 m0, %[i]\n\t"
        "s_or_b32 %[t], %[kd], 0x80000000\n\t"
        "v_writelane_b32 %[l0], %[t], m0\n"
        "3:\n"                                                              // kd = the node's low key half, id + 1
        HNSW_HOP_ADJACENCY
        HNSW_HOP_FILTER_ISSUE
        HNSW_PROBE(1)
        // the next nearest unexpanded member of W: its row is fetched now, beside this hop's vectors
        "s_cmp_eq_u64 %[um0], 0\n\t"
        "s_cbranch_scc1 7f\n\t"
        "s_ff1_i32_b64 %[i], %[um0]\n\t"
        "v_readlane_b32 %[pref], %[l0], %[i]\n"
        HNSW_HOP_PREFETCH_LOAD
        HNSW_HOP_FILTER_COMPACT
        HNSW_PROBE(2)
        HNSW_LOOP_ROUND_COMMON
        "50:\n\t"
        HNSW_PROBE(3)
        HNSW_INSERT_LOOP
        HNSW_PROBE(4)
        HNSW_LOOP_AFTER_INSERT
        // ---- behind the loop: the ways less often taken
        "2:\n\t"                                                            // pop from the upper slot
        "s_cmp_eq_u64 %[um1], 0\n\t"
        "s_cbranch_scc1 90f\n\t"
        "s_ff1_i32_b64 %[i], %[um1]\n\t"
        "v_readlane_b32 %[kd], %[l1], %[i]\n\t"
        "s_bitset0_b64 %[um1], %[i]\n\t"
        "s_mov_b32 m0, %[i]\n\t"
        "s_or_b32 %[t], %[kd], 0x80000000\n\t"
        "v_writelane_b32 %[l1], %[t], m0\n\t"
        "s_branch 3b\n"
        "7:\n\t"                                                            // the next one is in the upper slot, or there is none
        "s_mov_b32 %[pref], -1\n\t"
        "s_cmp_eq_u64 %[um1], 0\n\t"
        "s_cbranch_scc1 9b\n\t"
        "s_ff1_i32_b64 %[i], %[um1]\n\t"
        "v_readlane_b32 %[pref], %[l1], %[i]\n\t"
        "s_branch 8b\n"
        HNSW_HOP_ADJACENCY_MISS
        HNSW_LOOP_ROUNDS_RARE
        HNSW_INSERT_RARE
        // ---- no unexpanded member of W: entries evicted while tied with max(W) are still candidates (:568)
        HNSW_VT_WAYS_RARE
        HNSW_SEM_RARE
        HNSW_HOP_TAIL
        // back to the flag-in-bit-0 form
        "\n\ts_mov_b32 m0, %[sm0]"
        "\n\tv_alignbit_b32 %[l0], %[l0], %[l0], 31"
        "\n\tv_alignbit_b32 %[l1], %[l1], %[l1], 31"
        : [h0] "+&v"(w.hi[0]), [h1] "+&v"(w.hi[1]), [l0] "+&v"(w.lo[0]), [l1] "+&v"(w.lo[1]),
          HNSW_LOOP_OUT_A
          [um0] "=&s"(um0), [um1] "=&s"(um1), [g0] "=&s"(g0),
          HNSW_LOOP_OUT_B HNSW_LOOP_OUT_BAIL
        : HNSW_LOOP_IN
#ifdef HNSW_ASM_DEBUG
          , [maxh] "s"(maxhops)
#endif
        : "vcc", "scc", "memory" HNSW_LOOP_ROW_CLOBBER HNSW_PROBE_CLOBBER);
#else                           /* ---- ... in three and more: the slot set HNSW_NS(...) */
    asm volatile(
        // low key halves inside the loop: id + 1 with the expanded flag in bit 31 (a rotation of the (id + 1) << 1 | flag the
        // rest of the kernel keeps): the unexpanded members are the non-negative ones, a node id is one subtraction away
        "s_mov_b32 %[sm0], m0\n\t"                                       // m0 (lane select of v_writelane) is handed back as it was: not a clobber
        HNSW_NS(ALIGN_IN)
        HNSW_LOOP_CONSTANTS
        HNSW_SEM_INIT
        HNSW_NS(MX_INIT)                                                  // the slots' maxima (distance halves)
        "s_mov_b32 %[pref], -1\n"
        HNSW_ASM_ALIGN_K(HNSW_NS(ALIGN_PAD))
        // ================================ one hop ================================
        "1:\n\t"
        HNSW_PROBE(0)
        // pop: the first unexpanded member of W (pop_min, :565) and its flag
        HNSW_NS(UM_INIT)
        HNSW_POP_SLOT0("%[um0]", "%[l0]", "61f")
        "3:\n"                                                          // kd = the node's low key half, id + 1
        HNSW_X_ADJACENCY
        HNSW_X_FILTER_ISSUE
        HNSW_PROBE(1)
        "s_mov_b32 %[pref], -1\n\t"
        HNSW_PEEK_SLOT0("%[um0]", "%[l0]", "71f")
        HNSW_X_PREFETCH_LOAD
        HNSW_X_FILTER_COMPACT
        HNSW_PROBE(2)
        HNSW_LOOP_ROUND_COMMON
        "50:\n\t"
        HNSW_PROBE(3)
        HNSW_NS(INSERT_LOOP)
        HNSW_PROBE(4)
        HNSW_LOOP_AFTER_INSERT
        // ---- behind the loop
        HNSW_NS(POP_CHAIN)
        HNSW_NS(PEEK_CHAIN)
        HNSW_X_ADJACENCY_MISS
        HNSW_LOOP_ROUNDS_RARE
        HNSW_NS(INSERT_RARE)
        HNSW_VT_WAYS_RARE
        HNSW_SEM_RARE
        HNSW_HOP_TAIL
        // back to the flag-in-bit-0 form
        "\n\ts_mov_b32 m0, %[sm0]"
        HNSW_NS(ALIGN_OUT)
        : HNSW_NS(WOUT)
          HNSW_LOOP_OUT_A
          HNSW_NS(UMOUT) HNSW_LOOP_UM_EXTRA_OUT
          HNSW_LOOP_OUT_B HNSW_NS(MXOUT) HNSW_LOOP_OUT_BAIL
        : HNSW_LOOP_IN
        : "vcc", "scc", "memory" HNSW_LOOP_ROW_CLOBBER HNSW_PROBE_CLOBBER);
#endif
    w.wmax = wmax; w.ovf_cnt = od == wmax ? (int)oc : 0;
    n_dist = nd; n_hops = nh; status = st;
#if HNSW_LOOP_SEM
    // left in the middle of a hop (label 98): what search_layer needs to finish it
    rs.pass = fresh; rs.ckey = ckey; rs.cid1 = cid;
    rs.total = (int)((lastad - (cand - 4u)) >> 2);
    rs.remaining = (int)cnt > 0 ? (int)cnt : 0;
#if HNSW_LOOP_ROWS == 3
    rs.node = (int)hopn - 1;
#endif
    return bail != 0;
#else
    return false;
#endif
    }
};
#if HNSW_LOOP_ROWS == 2
#undef HNSW_B8_DOTS
#undef HNSW_B8_DOTS_N4
#undef HNSW_B8_COMBINE
#undef HNSW_B8_KEY
#endif
#if HNSW_LOOP_ROWS != 2
#undef HNSW_F32_ROW_LOAD
#undef HNSW_F32_ID_READ0
#undef HNSW_F32_ID_READN
#undef HNSW_F32_LG0
#undef HNSW_F32_LG1
#undef HNSW_F32_LG2
#undef HNSW_F32_LG3
#undef HNSW_F32_RAG_ON
#undef HNSW_F32_RAG_OFF
#undef HNSW_F32_RAG2_ON
#undef HNSW_F32_RAG3_ON
#undef HNSW_F32_ROUND_PICK
#undef HNSW_F32_VM1B
#undef HNSW_FX_BS
#undef HNSW_F32_DIST
#undef HNSW_F32_SUM
#undef HNSW_F32_KEY
#endif
#undef HNSW_X_ADJACENCY
#undef HNSW_X_ADJACENCY_MISS
#undef HNSW_X_FILTER_ISSUE
#undef HNSW_X_FILTER_COMPACT
#undef HNSW_X_PREFETCH_LOAD
#undef HNSW_X_DECL
#undef HNSW_X_SETS
#undef HNSW_X_OUT
#undef HNSW_X_IN
#if HNSW_LOOP_BLK
#undef HNSW_BLK_REG_0
#undef HNSW_BLK_REG_1
#undef HNSW_BLK_REG_2
#undef HNSW_BLK_REG_3
#undef HNSW_BLK_REG_4
#undef HNSW_BLK_REG_5
#undef HNSW_BLK_REG_6
#undef HNSW_BLK_REG_7
#undef HNSW_BLK_REG_8
#undef HNSW_BLK_REG_9
#undef HNSW_BLK_REG_10
#undef HNSW_BLK_REG_11
#undef HNSW_BLK_REG_12
#undef HNSW_BLK_REG_13
#undef HNSW_BLK_REG_14
#undef HNSW_BLK_DIR_READ
#undef HNSW_BLK_ZERO
#undef HNSW_BLK_CLEAR
#endif
#undef HNSW_LOOP_BLK
#undef HNSW_LOOP_VT3
#undef HNSW_LOOP_TSH_OPERAND
#undef HNSW_VT_WAYS_TEST
#undef HNSW_VT_WAYS_JOIN
#undef HNSW_VT_SHIFT
#undef HNSW_VT_WAYS_RARE
#undef HNSW_SPLIT_HOP
#undef HNSW_SPLIT_COMPACT
#undef HNSW_SEM_ACCEPT
#undef HNSW_SEM_REJECT
#undef HNSW_EVICT_TIE
#undef HNSW_SEM_RARE
#undef HNSW_SEM_INIT
#undef HNSW_LOOP_SEM
#undef HNSW_LOOP_NCH
#undef HNSW_LOOP_CONSTANTS
#undef HNSW_LOOP_ROUND_COMMON
#undef HNSW_LOOP_ROUNDS_RARE
#undef HNSW_LOOP_AFTER_INSERT
#undef HNSW_NS_CAT2
#undef HNSW_NS_CAT
#undef HNSW_NS
#undef HNSW_LOOP_UM_EXTRA_DECL
#undef HNSW_LOOP_UM_EXTRA_OUT
#undef HNSW_LOOP_ROW_OUT
#undef HNSW_LOOP_D_OUT
#undef HNSW_LOOP_OUT_A
#undef HNSW_LOOP_OUT_B
#undef HNSW_LOOP_OUT_BAIL
#undef HNSW_LOOP_QUERY_IN
#undef HNSW_LOOP_ROW_IN
#undef HNSW_LOOP_ROW_CLOBBER
#undef HNSW_LOOP_IN
#undef HNSW_LOOP_NSLOT
#undef HNSW_LOOP_ROWS
#undef HNSW_LOOP_METRIC
