// switches.hpp -- every GRLBWT_* environment switch the library reads, declared once.
//
// A switch chooses between forms of one computation (the tests force most of them and compare the image with the oracle:
// none changes the output), lowers a limit so that small inputs take a large-input branch, or turns on a trace.
// Entry: X(name, field, type, default, meaning).  The type is the kind: bool = a flag (set to anything: on), int / u64 = an
// integer (atoi / atoll of the value), char = a word of which only the first letter counts (0: unset).
//
// Tiers:
//   product  read by the device library at the entry of every C-API call (prim::sw(): the snapshot guarded() takes in capi_impl.hpp)
//   init     read by the device library once per process (prim::init_sw()): they configure the runtime and the allocator
//   test     the CPU test suites' switches -- older forms of the collection-level flow kept as references for the multi-rank tests,
//            limits lowered so that small inputs take a branch, fault injection.  Compiled in only where GRLBWT_PRIM_HIP is not
//            defined, i.e. over the serial stand-in of the primitives (tests/hostsim): the device library (prim_hip.hpp defines it
//            before including this file) has their defaults as constants and their names do not reach its binary
//   dev      experiment switches (tile shapes, alternative kernels measured against each other): compiled in only with
//            -DGRLBWT_DEV_SWITCHES (tools/build_dev.sh); constants, and not in the binary, elsewhere
#pragma once
#include <cstdint>
#include <cstdlib>

#define GRLBWT_SWITCHES_PRODUCT(X)                                                                                                 \
    X(GRLBWT_PART_MIN_OCC, part_min_occ, uint64_t, (uint64_t)1 << 20, "smallest level (phrase occurrences) that takes the partitioned naming") \
    X(GRLBWT_PART_BITS, part_bits, int, 0, "partition bits of the partitioned naming, 1..20 (0: from the level's size)")          \
    X(GRLBWT_PART_ONE_PASS, part_one_pass, bool, false, "partitioned naming: records and long phrases in one pass through the table") \
    X(GRLBWT_FORCE_DIRECT_INDEX, force_direct_index, bool, false, "take the direct index on texts too small for a sample")        \
    X(GRLBWT_TABLE_TRACE, table_trace, bool, false, "trace the phrase-table and cell-layout decisions on stderr")                 \
    X(GRLBWT_A2A_SELF_VIA_COMM, a2a_self_via_comm, bool, false, "a rank's own all-to-all block goes through the callback too")    \
    X(GRLBWT_RUN_KEYS_MIN, run_keys_min, uint64_t, 512, "phrase length from which the suffix sort takes run-aware keys")         \
    X(GRLBWT_DOUBLING_AFTER, doubling_after, uint64_t, 24, "refinement rounds of a long-phrase level before doubling rounds")     \
    X(GRLBWT_BASE_CASE_RATIO, base_case_ratio, uint64_t, 5, "a whole build stops parsing at a level of at most this many cells per string and sorts its suffixes (0: never)") \
    X(GRLBWT_SEG_CAP, seg_cap, int, 64, "largest suffix group ordered by counting (kSegCap); larger ones in LDS or by two radix sorts") \
    X(GRLBWT_SEG_LDS_CAP, seg_lds_cap, int, 4096, "largest suffix group ordered in LDS (above: two radix sorts; 0: no LDS tier)") \
    X(GRLBWT_CELL_LAYOUT, cell_layout, char, 0, "p[acked] | s[eparate]: a wider induction cell layout than the input needs")     \
    X(GRLBWT_NO_CELL32, no_cell32, bool, false, "induction cells of one word in 64 bits even where 32 would do")               \
    X(GRLBWT_ASM_TWO_PASS, asm_two_pass, bool, false, "pass C always as count + emit (no one-walk form)")                       \
    X(GRLBWT_ASM_ONE_WALK, asm_one_walk, bool, false, "pass C tries the one-walk form at every level, plain or not")           \
    X(GRLBWT_ASM_IMAGE, asm_image, int, 1, "level 0's pass C writes the .rl_bwt records itself (0: emit + pack)")             \
    X(GRLBWT_DIST_GATHERED_DICT, dist_gathered_dict, bool, false, "multi-rank: the dictionary gathered on every rank, not sharded") \
    X(GRLBWT_DIST_SHARDED_DICT_MIN, dist_sharded_dict_min, int, 4, "multi-rank: ranks from which the dictionary is sharded")    \
    X(GRLBWT_DIST_SHARDED_DICT_MIN_SYMS, dist_sharded_dict_min_syms, uint64_t, (uint64_t)1 << 27, "multi-rank: dictionary symbols from which it is sharded") \
    X(GRLBWT_INVERT, invert, char, 0, "r[uns] | p[ositions]: the form of the inversion (unset: by the memory it needs)")         \
    X(GRLBWT_XS_MAXC, xs_maxc, int, 32, "most cells per item the fused expansion sort takes (lower: the unfused branch)")        \
    X(GRLBWT_ALPHA_TABLE_BITS, alpha_table_bits, int, 20, "log2 of the slots of the alphabet compaction's table, 2..26 (lower: the sorting regime)") \
    X(GRLBWT_FM_TOP_BITS, fm_top_bits, int, 12, "log2 of the keys of an FM index's search array kept in LDS, 0..12 (0: none; lower: small indexes search HBM)") \
    X(GRLBWT_FM_MATCH, fm_match, char, 0, "l[anes]: grlbwt_fm_match / grlbwt_fm_mems with one lane per query cell, grlbwt_fm_approx with one lane per pattern, and no refilling, not lanes that take tickets") \
    X(GRLBWT_WALK_LANES, walk_lanes, uint64_t, 0, "most lanes of a checkpointed walk launch, rounded up to a wave (0: from occupancy; lower: small inputs refill their lanes)") \
    X(GRLBWT_MERGE_ROUND, merge_round, char, 0, "s[ort]: a round of the image merge as gathered keys and a stable sort, not the fused kernels") \
    X(GRLBWT_LCP_ROUND, lcp_round, char, 0, "p[lain]: a pass of grlbwt_fm_lcp through the generic primitives, not the fused kernel")  \
    X(GRLBWT_IO_THREADS, io_threads, int, 0, "reader / writer threads per file chunk, 1..64 (0: from the host's cores)")         \
    X(GRLBWT_QUIET_ENV, quiet_env, bool, false, "no note on stderr about the switches set in the environment")

#define GRLBWT_SWITCHES_INIT(X)                                                                                                     \
    X(GRLBWT_TRACE, trace, char, 0, "1: print every launch and synchronise after it")                                          \
    X(GRLBWT_SYNC_SITES, sync_sites, bool, false, "profile: count behind which launch site the host waited")                  \
    X(GRLBWT_MEM_TRACE, mem_trace, bool, false, "per-stage peak device memory on stderr")                                      \
    X(GRLBWT_POOL_CLASSIC, pool_classic, bool, false, "hipMalloc slabs only, no reserved arena")                              \
    X(GRLBWT_POOL_TRACE, pool_trace, bool, false, "what backing the arena cost the process, on stderr at exit")               \
    X(GRLBWT_IO_TRACE, io_trace, bool, false, "where the file loader and the image writer spend their time, on stderr")

#define GRLBWT_SWITCHES_TEST(X)                                                                                                     \
    X(GRLBWT_NO_DIRECT_INDEX, no_direct_index, bool, false, "the hot table instead of the direct index")                       \
    X(GRLBWT_NO_HOT_TABLE, no_hot_table, bool, false, "no hot table in front of the phrase table")                            \
    X(GRLBWT_A2A_BLOCK, a2a_block, uint64_t, (uint64_t)256 << 20, "bytes of one all-to-all block before it goes in rounds")   \
    X(GRLBWT_TEST_DICT_PART_PAD, test_dict_part_pad, uint64_t, 0, "offset added to the global numbering of the dictionary parts") \
    X(GRLBWT_DIST_REC_ROUND_TRIP, dist_rec_round_trip, bool, false, "sharded sort: records travel back and forth, not carried") \
    X(GRLBWT_SORT_EXCHANGE_MIN, sort_exchange_min, int, 4, "ranks from which the sharded sort exchanges its first keys")     \
    X(GRLBWT_DIST_REC_FLY_MIN, dist_rec_fly_min, int, 8, "ranks from which the group records are made on the fly")           \
    X(GRLBWT_DIST_REPLICATED_PREBWT, dist_replicated_prebwt, bool, false, "every rank holds the whole pre-BWT")               \
    X(GRLBWT_DIST_REPLICATED_INDUCTION, dist_replicated_induction, bool, false, "the induction replicated on every rank")      \
    X(GRLBWT_DIST_REPLICATED_GRAMMAR, dist_replicated_grammar, bool, false, "the grammar passes replicated on every rank")     \
    X(GRLBWT_DIST_REPLICATED_DICT, dist_replicated_dict, bool, false, "the dictionary stage replicated on every rank")         \
    X(GRLBWT_GRAMMAR_JUMP, grammar_jump, bool, false, "the grammar walks jump to their stops whatever the phrase lengths")     \
    X(GRLBWT_MERGE_CELLS, merge_cells, char, 0, "s[ort]: the received induction cells merged by a radix sort, not by blocks") \
    X(GRLBWT_TEST_FAIL_RANK, test_fail_rank, int, -1, "this rank fails in the phrase hashing")                                \
    X(GRLBWT_TEST_FAIL_RANK_SORT, test_fail_rank_sort, int, -1, "this rank fails in the suffix refinement")                 \
    X(GRLBWT_TEST_FAIL_RANK_MERGE, test_fail_rank_merge, int, -1, "this rank fails in the phrase merge")                    \
    X(GRLBWT_TEST_FAIL_RANK_INDUCE, test_fail_rank_induce, int, -1, "this rank fails in the induction")

#define GRLBWT_SWITCHES_DEV(X)                                                                                                      \
    X(GRLBWT_NOPOOL, nopool, bool, false, "no slab allocator: hipMalloc / hipFree for every buffer")                           \
    X(GRLBWT_NO_PART, no_part, bool, false, "no partitioned naming (single GPU)")                                              \
    X(GRLBWT_DIST_NO_PART, dist_no_part, bool, false, "no partitioned naming (multi-rank)")                                   \
    X(GRLBWT_NO_NAME_STREAM, no_name_stream, bool, false, "the direct index without the name_stream kernel")                  \
    X(GRLBWT_SORT_KMAX, sort_kmax, int, 16, "most symbols in the first suffix sort's key")                                     \
    X(GRLBWT_FOR_EACH_GRID, for_each_grid, char, 0, "f[ixed]: 8 workgroups per CU; anything else: twice the resident number") \
    X(GRLBWT_SPAN_BLOCKS_PER_CU, span_blocks_per_cu, uint64_t, 0, "workgroups per CU of the span kernels (0: from occupancy)") \
    X(GRLBWT_SORT_DIGIT, sort_digit, int, 8, "widest radix digit of the sorts, 8..10 bits")                                    \
    X(GRLBWT_XS_DIGIT8, xs_digit8, bool, false, "the expansion sort keeps 8-bit digits where 9 would save a pass")            \
    X(GRLBWT_RS_THREADS, rs_threads, int, 0, "threads per workgroup of the radix sorts (0: by record width)")                \
    X(GRLBWT_RS_THREADS_XS, rs_threads_xs, int, 0, "the same for the sorts behind the fused expansion")                      \
    X(GRLBWT_SM_SPT, sm_spt, int, 0, "segments per thread of the segment merge, 4 or 8 (0: by the level)")                  \
    X(GRLBWT_DEV_SM1_SPT, dev_sm1_spt, int, 0, "segments per thread of the one-walk pass C, 4 or 8 (0: by the level)")      \
    X(GRLBWT_DEV_WALK_STORES, dev_walk_stores, char, 0, "c[ells]: the checkpointed write walk stores u8/u16 cells one by one, not collected as aligned 8-byte words") \
    X(GRLBWT_DEV_OVERLAP_EXPAND, dev_overlap_expand, char, 0, "f[or_each]: grlbwt_fm_overlap_targets as a for_each with a search per entry, not the tile kernel") \
    X(GRLBWT_DEV_KMER_DECODE, dev_kmer_decode, char, 0, "f[or_each]: the table of grlbwt_fm_kmers through for_each_set_bit, one lane per entry storing its own cells, not the tile kernel") \
    X(GRLBWT_DEV_KMER_MATES, dev_kmer_mates, char, 0, "f[or_each]: the mate pass of grlbwt_fm_kmers_canonical through for_each_set_bit over the heads, one lane per head without a top level and the complement table in memory, not the ticket kernel") \
    X(GRLBWT_DEV_DOCS_TILE, dev_docs_tile, char, 0, "f[or_each]: grlbwt_docs_count / grlbwt_docs_list through bitvector_from_pred and for_each_set_bit with a search per range row and per entry, not the tile kernels (entries with occurrences always are)") \
    X(GRLBWT_DEV_REPEAT_SEARCH, dev_repeat_search, char, 0, "f[or_each]: the counting and the selection of grlbwt_fm_repeats through reduces and bitvector_from_pred with searches in the tree in memory, the levels by for_each, not the tile and the minima kernel") \
    X(GRLBWT_DEV_DEBRUIJN, dev_debruijn, char, 0, "f[or_each]: the first cells of the unitigs of grlbwt_debruijn_unitigs through a for_each over the nodes, not the tile kernel") \
    X(GRLBWT_DEV_CDEBRUIJN, dev_cdebruijn, char, 0, "f[or_each]: the merge of grlbwt_cdebruijn_create through a reduce, a scan and a for_each over the sorted records, and the first cells of grlbwt_cdebruijn_unitigs through a for_each over the nodes with the walks inline, not the tile kernels and the tickets") \
    X(GRLBWT_DEV_LB_PATIENCE,dev_lb_patience, uint64_t, 200000000, "clock ticks a look-back tile waits before it gives up")

namespace prim {

struct Switches {
#define GRL_SW_FIELD(name, field, type, def, meaning) type field = def;
#define GRL_SW_CONST(name, field, type, def, meaning) static constexpr type field = def;
    GRLBWT_SWITCHES_PRODUCT(GRL_SW_FIELD)
    GRLBWT_SWITCHES_INIT(GRL_SW_FIELD)
#ifndef GRLBWT_PRIM_HIP
    GRLBWT_SWITCHES_TEST(GRL_SW_FIELD)
#else
    GRLBWT_SWITCHES_TEST(GRL_SW_CONST)
#endif
#ifdef GRLBWT_DEV_SWITCHES
    GRLBWT_SWITCHES_DEV(GRL_SW_FIELD)
#else
    GRLBWT_SWITCHES_DEV(GRL_SW_CONST)
#endif
#undef GRL_SW_FIELD
#undef GRL_SW_CONST

    static void parse(bool &v, const char *) { v = true; }
    static void parse(int &v, const char *e) { v = atoi(e); }
    static void parse(uint64_t &v, const char *e) { v = (uint64_t)atoll(e); }
    static void parse(char &v, const char *e) { v = e[0]; }
    // f(name) for every switch compiled into this build
    template <class F>
    static void for_each_name(F f) {
#define GRL_SW_NAME(name, field, type, def, meaning) f(#name);
        GRLBWT_SWITCHES_PRODUCT(GRL_SW_NAME)
        GRLBWT_SWITCHES_INIT(GRL_SW_NAME)
#ifndef GRLBWT_PRIM_HIP
        GRLBWT_SWITCHES_TEST(GRL_SW_NAME)
#endif
#ifdef GRLBWT_DEV_SWITCHES
        GRLBWT_SWITCHES_DEV(GRL_SW_NAME)
#endif
#undef GRL_SW_NAME
    }
    static Switches from_env() {
        Switches s;
#define GRL_SW_READ(name, field, type, def, meaning) if (const char *e = getenv(#name)) parse(s.field, e);
        GRLBWT_SWITCHES_PRODUCT(GRL_SW_READ)
        GRLBWT_SWITCHES_INIT(GRL_SW_READ)
#ifndef GRLBWT_PRIM_HIP
        GRLBWT_SWITCHES_TEST(GRL_SW_READ)
#endif
#ifdef GRLBWT_DEV_SWITCHES
        GRLBWT_SWITCHES_DEV(GRL_SW_READ)
#endif
#undef GRL_SW_READ
        return s;
    }
};

// The snapshot of the current C-API call: taken on entry (take_switches), read by the engine and the primitives through sw().
inline Switches &call_switches() {
    static Switches s;
    return s;
}
inline const Switches &sw() { return call_switches(); }
inline void take_switches() { call_switches() = Switches::from_env(); }
// The init tier: the environment the process had when the runtime or the allocator first asked (they cannot change afterwards).
inline const Switches &init_sw() {
    static const Switches s = Switches::from_env();
    return s;
}

}   // namespace prim
