// hnsw_hop_instances.inc -- WHICH shapes have a hand-scheduled layer-0 loop: the explicit specialisations
// HopLoop<NCH, NSLOT, METRIC, ROWS, SEM, BLK> (hnsw_hop_asm.hip.h), one stanza each, written by hand; every other shape is the
// primary template and keeps search_layer's C++ loop.  This table is the statement: comments elsewhere point here.
//
// A translation unit of hnsw_search_variants.hip is compiled per (metric, accept rule, row format), and hnsw_hop_loop.inc takes
// METRIC, SEM and ROWS from that unit's HNSW_V_METRIC / HNSW_V_SEMF / HNSW_V_FULL: a stanza states what varies inside a unit.
//   NCH    2: rows of 65..128 dimensions; 4: rows of 129..256
//   NSLOT  1, 2, 3, 4, 6, 8 key registers per lane that hold W (ef <= 64 / 128 / 192 / 256 / 384 / 512)
//   BLK    1: Visited as bitmap blocks instead of the tag cache (left out: 0) -- W in three or more registers only, and not the
//          byte rows of 129..256 dimensions
// Per unit: byte rows (HNSW_V_FULL 2) 16 shapes; float32 rows ragged / full / split (0 / 1 / 3) 20 each; half rows (4) and every
// unit without HNSW_V_METRIC (builder, layer operators, ordering, scan: row format decided at run time) none.  Over two metrics
// and two rules that is 4 x (16 + 3 x 20) = 304.  A new slot count is one stanza (two with its BLK 1) under each NCH; a new row
// format is a value of HNSW_V_FULL that hnsw_hop_loop.inc knows as HNSW_LOOP_ROWS.  The order is the order the kernels are
// compiled in: keep it.
#if defined(HNSW_V_METRIC) && HNSW_V_FULL != 4

// ---- rows of 65..128 dimensions
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 1
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 2
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 3
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 3
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 4
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 4
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 6
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 6
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 8
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 2
#define HNSW_LOOP_NSLOT 8
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"

// ---- rows of 129..256 dimensions (bitmap blocks: the float32 rows only)
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 1
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 2
#include "hnsw_hop_loop.inc"
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 3
#include "hnsw_hop_loop.inc"
#if HNSW_V_FULL != 2
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 3
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"
#endif
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 4
#include "hnsw_hop_loop.inc"
#if HNSW_V_FULL != 2
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 4
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"
#endif
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 6
#include "hnsw_hop_loop.inc"
#if HNSW_V_FULL != 2
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 6
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"
#endif
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 8
#include "hnsw_hop_loop.inc"
#if HNSW_V_FULL != 2
#define HNSW_LOOP_NCH 4
#define HNSW_LOOP_NSLOT 8
#define HNSW_LOOP_BLK 1
#include "hnsw_hop_loop.inc"
#endif

#endif
