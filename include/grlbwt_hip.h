/*
 * grlbwt_hip.h -- C-ABI of the MI355X-native BCR-BWT engine (libgrlbwt_hip.so).
 *
 * Drop-in boundary for the parse-then-induce hot path of ddiazdom/grlBWT.  The
 * reference has no FFI/plugin interface: its seam for this
 * path is the pair of C++ entry points called by grl_bwt_algo
 * (include/grl_bwt.hpp:23-79):
 *
 *     size_t exact_algo::par_phase<sym_type>(i_file, n_threads, hbuff_frac, ws)   lib/exact_algo/exact_par_phase.cpp:285-372
 *     void   exact_algo::ind_phase<b_f_r>(ws, p_round)                            lib/exact_algo/exact_ind_phase.cpp:674-697
 *
 * plus the file formats at both ends (raw cells in, `.rl_bwt` out, include/bwt_io.h).
 * Each entry point below names the reference function(s) it replaces.  Plain C
 * types only; one context per GPU; calls on one context must be serialised by the
 * caller; every function returns 0 or a negative GRLBWT_E* code, never throws and
 * never exits; host buffers are borrowed for the duration of the call; device
 * buffers are owned by the context and released by grlbwt_ctx_destroy.
 *
 * There is no CPU fallback: without a usable HIP device grlbwt_ctx_create fails
 * with GRLBWT_EDEVICE.
 *
 * Process model: ONE context (= one GPU) per process, as in the one-process-per-GPU launch of
 * torch.distributed; the device, the engine's HIP stream and its slab allocator are process-wide.
 * The engine runs on its own non-blocking stream: data handed over with grlbwt_text_attach_device must
 * be complete (synchronise the producing stream first), results are complete when a call returns.
 */
#ifndef GRLBWT_HIP_H
#define GRLBWT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRLBWT_ABI_VERSION 3

#define GRLBWT_OK 0
#define GRLBWT_EINVAL (-22)     /* bad argument / call out of order                                  */
#define GRLBWT_EDEVICE (-5)     /* HIP runtime error (no device, launch failure, ...)                */
#define GRLBWT_ENOMEM (-12)     /* device or host allocation failed                                  */
#define GRLBWT_EILLFORMED (-84) /* reference: "Error: the file is ill formed", exit(1) (utils.cpp:177-180) */
#define GRLBWT_ERANGE (-75)     /* input beyond what this build supports -- the limits, all checked:
                                 *   collection            < 2^40 cells (64-bit positions from 2^32 - 256 cells on);
                                 *   symbols: any value up to 2^64 - 5 (the header width comes from max_sym + 4), fewer than 2^30 - 16 DISTINCT ones --
                                 *   a text with a symbol of 2^30 - 8 or more is built on the ranks of its values (grlbwt_alphabet_size),
                                 *   single-GPU only: grlbwt_dist_build refuses it on every rank;
                                 *   the alphabet of every level >= 1 (metasymbols of a round)               < 2^30;
                                 *   distinct phrases of one round < 2^32, their symbols (the round's dictionary) < 2^32
                                 *   (collection-level mode: per rank's part of the merged dictionary and per key range of its
                                 *   suffixes, while every phrase frequency is < 2^32 and no phrase has >= 512 cells);
                                 *   phrase-table slots of one round <= 2^31 (2^30 with the hot table of level 0);
                                 *   phrase OCCURRENCES of one round: no bound of their own in the 64-bit build (level 0 of a
                                 *   24.9 GB collection has 7.3 G); a shard of the collection-level mode < 2^32 per round.
                                 * The reference takes dictionaries up to 64-bit suffix-array cells (exact_par_phase.cpp:244-263). */
#define GRLBWT_ENOSPC (-28)     /* phrase table overflow                                              */
#define GRLBWT_EINTERNAL (-71)  /* internal consistency check failed                                  */
#define GRLBWT_ENOTDNA (-86)    /* reference: "The input seems not to be DNA (invalid symbol:X)", exit(1) (fastx_handler.cpp:30-33) */

/* ctx flags */
#define GRLBWT_FLAG_KEEP_LEVELS 1u   /* keep every level's text and BWT for parity inspection        */
#define GRLBWT_FLAG_SYNC_DEBUG 2u    /* synchronise after every kernel launch (fault localisation)   */
#define GRLBWT_FLAG_FORCE_IDX64 4u   /* 64-bit positions/lengths whatever the input size (sharded collections, tests) */
#define GRLBWT_FLAG_CLASSIC_POOL 8u  /* device memory from hipMalloc slabs, not from the on-demand virtual-memory arena:
                                      * for buffers that are handed to a communication library (multi-process RCCL) */

typedef struct grlbwt_ctx grlbwt_ctx;

/* collection_stats<T> result (external/cdt/lib/utils.cpp:100-189, include/utils.h:20-28) + final header */
typedef struct grlbwt_stats {
    uint64_t n_strings, n_syms, min_sym, max_sym, max_sym_freq;
    uint64_t sb, fb;            /* bytes per run symbol / run length in the final .rl_bwt */
} grlbwt_stats;

/* the "Stats:" block of par_round (lib/exact_algo/exact_par_phase.cpp:484-488) */
typedef struct grlbwt_round_info {
    uint64_t n_in;              /* cells of the round's input text                  */
    uint64_t n_phrases;         /* "Parsing phrases" (distinct)                     */
    uint64_t dict_syms;         /* "Number of symbols in the phrases"               */
    uint64_t n_metasyms;        /* "Number of unsolved BWT blocks" (tot_phrases)    */
    uint64_t parse_size;        /* "Parse size"                                     */
    uint64_t sigma;             /* alphabet size of the input text of the round     */
    uint64_t max_phrase_len, sort_iters;
} grlbwt_round_info;

/* the "Stats:" block of infer_lvl_bwt (lib/exact_algo/exact_ind_phase.cpp:372-384) + kernel shape */
typedef struct grlbwt_level_info {
    uint64_t n;                 /* "BWT size (n)"                                   */
    uint64_t n_runs;            /* "Number of runs (r)"                             */
    uint64_t runs_next;         /* runs of BWT_{r+1} scanned                        */
    uint64_t induced_cells;     /* chain steps + TAKE cells scattered (pass B)      */
    uint64_t prebwt_runs, segments, atoms;
    /* SURVEY 8d's E'_r (grammar-chain steps) and E_r (cells after the in-bucket merge = n_runs of compute_hocc_size,
     * exact_ind_phase.cpp:42-109); counted only while grlbwt_profile_enable(1) is on, else 0 */
    uint64_t chain_steps, merged_cells;
} grlbwt_level_info;

/* wall-clock seconds per stage (stream-synchronised) and algorithmic byte counts */
typedef struct grlbwt_counters {
    double t_stats, t_classify, t_hash, t_dict_sort, t_dict_groups, t_emit;
    double t_ind_expand, t_ind_split, t_ind_assemble, t_finish;
    uint64_t bytes_classify_hash;   /* sum_r n_r*w_r  (one read of every level's text per scan) */
    uint64_t bytes_emit;            /* sum_r n_{r+1}*4 written + read back                                 */
    uint64_t bytes_induce_scatter;  /* sum_r R_{r+1}*(4+idx) + E_r*(4+idx)   (pass A+B formula) */
    uint64_t bytes_induce_assemble; /* sum_r P_r + E_r + R_{r+1} read + R_r written, (4+idx) B each        */
    uint64_t idx_bytes;             /* 4 or 8: width of positions/lengths in HBM for this input            */
} grlbwt_counters;

/* ---- lifetime ------------------------------------------------------------ */
int grlbwt_abi_version(void);
/* "hip-gfx950" for the product library.  (The serial stand-in that the CPU test-suite builds under
 * tests/hostsim answers "serial-test-standin"; the host mirrors refuse it unless a test asks for it.) */
const char *grlbwt_backend_name(void);
const char *grlbwt_strerror(int code);
/* last error message of this context (valid until the next call on it) */
const char *grlbwt_last_error(const grlbwt_ctx *ctx);
/* replaces tmp_workspace construction in run_int (main.cpp:80-96): all level files
 * of the reference's workspace become device buffers owned by the context.       */
int grlbwt_ctx_create(int device_id, uint32_t flags, grlbwt_ctx **out);
void grlbwt_ctx_destroy(grlbwt_ctx *ctx);
/* run the engine's kernels on a caller-provided hipStream_t (e.g. torch's current stream) */
int grlbwt_ctx_set_stream(grlbwt_ctx *ctx, void *hip_stream);

/* ---- input: replaces collection_stats<sym_type>(i_file) (utils.cpp:100-189) and
 * the i_file_stream reads of the first round (file_streams.hpp:93-105) ---------- */
/* copy n_cells cells of cell_bytes in {1,2,4,8} from host memory to HBM and scan them */
int grlbwt_text_upload(grlbwt_ctx *ctx, const void *host_cells, uint64_t n_cells, int cell_bytes);
/* the same from a file of raw cells (the reference's i_file_stream + collection_stats, file_streams.hpp:93-105,
 * utils.cpp:100-189): chunks are read into pinned staging buffers by reader threads and copied to HBM while the next
 * chunk is read; for byte cells the symbol histogram is taken per chunk on the device behind the copies.  A file whose
 * size is 0 or not a multiple of cell_bytes is ill formed (GRLBWT_EILLFORMED). */
int grlbwt_text_load_file(grlbwt_ctx *ctx, const char *path, int cell_bytes);
/* the same for bytes [offset_bytes, offset_bytes + n_bytes) of the file: a record shard of the collection-level mode
 * (the caller cuts at record boundaries; both numbers are multiples of cell_bytes) */
int grlbwt_text_load_file_range(grlbwt_ctx *ctx, const char *path, uint64_t offset_bytes, uint64_t n_bytes, int cell_bytes);
/* use cells already resident in HBM (borrowed until the context is reset/destroyed; 16-byte aligned).  The statistics are
 * taken here: the buffer must not change between this call and the end of the build (a build that finds a cell value in it
 * that was not there fails with GRLBWT_EINVAL; other changes give the image of neither text). */
int grlbwt_text_attach_device(grlbwt_ctx *ctx, const void *dev_cells, uint64_t n_cells, int cell_bytes);
int grlbwt_get_stats(const grlbwt_ctx *ctx, grlbwt_stats *out);

/* ---- wide symbols: the BWT depends only on the order and the equality of the symbols, so a text of 4- or 8-byte cells with a
 * symbol of 2^30 - 8 or more is replaced, when it is loaded, by the ranks of its values among its distinct values; the
 * statistics and the image carry the values.  With GRLBWT_FLAG_KEEP_LEVELS everything at level 0 of such a build is in RANK
 * space: round_info[0].sigma is the number of distinct values, the grammar cells, the pre-BWT and the level-0 BWT of the
 * stage-wise inspection hold ranks (the separator is rank 0) and codes above them.
 * grlbwt_alphabet_size: *n_distinct = 0 when the loaded text was not compacted.  grlbwt_alphabet_download: the sorted values. */
int grlbwt_alphabet_size(const grlbwt_ctx *ctx, uint64_t *n_distinct);
int grlbwt_alphabet_download(const grlbwt_ctx *ctx, uint64_t *values_out);
/* the compaction alone, device buffer to device buffer: dev_ranks_u32[i] = the rank of cell i (n_cells words), dev_values_u64 =
 * the sorted distinct values (GRLBWT_EINVAL when there are more than capacity_values; *n_distinct is set all the same).
 * cell_bytes 4 or 8. */
int grlbwt_alphabet_compact_device(grlbwt_ctx *ctx, const void *dev_cells, uint64_t n_cells, int cell_bytes, void *dev_ranks_u32,
                                   void *dev_values_u64, uint64_t capacity_values, uint64_t *n_distinct);

/* ---- FASTA/FASTQ ingestion: replaces is_fastx / check_gzip (external/cdt/lib/utils.cpp:13-30,53-60)
 * and fastx2plain_format (external/bioparsers/lib/fastx_handler.cpp:7-58, kseq.h:179-220), which the reference's
 * main.cpp:118-136 has switched off.  The file (gzip members are inflated on the host) goes to HBM as it is; the records
 * become the one-string-per-line text on the device: every record's sequence lines joined, '\n' behind it, and with
 * GRLBWT_FASTX_REVCOMP its reverse complement + '\n' as a second string (a symbol outside ACGT: GRLBWT_ENOTDNA, with the
 * reference's message naming the symbol).  FASTA with any line wrapping and four-line FASTQ are classified in parallel;
 * other layouts (FASTQ over several lines, damaged records) are walked record by record like kseq does, with kseq's
 * outcome (a record whose quality string has the wrong length ends the conversion). */
#define GRLBWT_FASTX_REVCOMP 1u
int grlbwt_fastx_probe(const char *path, int *is_fastx, int *is_gz);
int grlbwt_text_load_fastx(grlbwt_ctx *ctx, const char *path, uint32_t fastx_flags, uint64_t *n_strings);
/* the conversion alone, device buffer to device buffer (capacity >= n_in, or 2 * n_in with reverse complements) */
int grlbwt_fastx_convert_device(grlbwt_ctx *ctx, const void *dev_in, uint64_t n_in, uint32_t fastx_flags, void *dev_out,
                                uint64_t capacity, uint64_t *n_out, uint64_t *n_strings);

/* ---- the order of the stage-wise calls -----------------------------------------
 * A context with a text is in one of five states: LOADED (no round has run), PARTLY PARSED, PARSED (the last round has
 * run), INDUCING (after grlbwt_induce_first, while a level is left to induce) and DONE (the image is there).  Loading a text
 * replaces everything the context held of the previous one and starts at LOADED; a load that fails leaves the context
 * without a text, and every call below returns GRLBWT_EINVAL until one is loaded.
 *
 *   grlbwt_parse_round    LOADED, PARTLY PARSED: one more round.  From PARSED on: GRLBWT_OK, *done = 1, nothing changes.
 *   grlbwt_parse_phase    LOADED, PARTLY PARSED: the rounds that are left.  From PARSED on: GRLBWT_OK, *n_rounds = the rounds
 *                         that have run, nothing changes.
 *   grlbwt_induce_first   PARSED: the deepest level's BWT, once per text.  Every other state: GRLBWT_EINVAL.
 *   grlbwt_induce_level   INDUCING: one level down; the call that produces level 0 also writes the image (DONE).  Every other
 *                         state: GRLBWT_EINVAL.
 *   grlbwt_induce_phase   LOADED, PARTLY PARSED: GRLBWT_EINVAL.  PARSED: the whole induction.  INDUCING: the levels that are
 *                         left, and the image.  DONE: GRLBWT_OK, nothing changes.
 *   grlbwt_build          from every state to DONE.  In DONE: GRLBWT_OK, the image is not written again (the same pointer,
 *                         the same bytes).  A build that does the parsing itself may stop it at a level of short strings
 *                         (GRLBWT_BASE_CASE_RATIO): grlbwt_parse_phase then reports fewer rounds than the stage-wise calls run.
 *   grlbwt_result_*       DONE: the image.  Every other state: GRLBWT_EINVAL.
 *
 * A call that is refused (GRLBWT_EINVAL) or has nothing to do changes nothing: the calls that follow produce what they would
 * have produced without it, and grlbwt_last_error names this refusal, not an earlier failure.  A stage call that fails after
 * it has begun to change a level (out of memory, a device error) ends the text: every stage and result call returns
 * GRLBWT_EINVAL until a text is loaded again.  A failure inside the first parsing round has changed nothing yet and leaves
 * the context in LOADED: a borrowed text that was found changed there (grlbwt_text_attach_device) builds once its bytes
 * are as they were. */

/* ---- parsing phase ------------------------------------------------------- */
/* one par_round (exact_par_phase.cpp:374-497): LMS breaks, phrase hashing, dictionary
 * sort, pre-BWT, grammar, parse emission.  *done = 1 after the last round (:496). */
int grlbwt_parse_round(grlbwt_ctx *ctx, grlbwt_round_info *info, int *done);
/* exact_algo::par_phase (exact_par_phase.cpp:285-372): all rounds; *n_rounds = rounds run */
int grlbwt_parse_phase(grlbwt_ctx *ctx, int *n_rounds);
int grlbwt_round_info_get(const grlbwt_ctx *ctx, int round, grlbwt_round_info *info);

/* ---- induction phase ------------------------------------------------------ */
/* parse2bwt (exact_ind_phase.cpp:603-672) */
int grlbwt_induce_first(grlbwt_ctx *ctx);
/* infer_lvl_bwt<b> (exact_ind_phase.cpp:111-386) for the next level down; *level = level produced.
 * The reference's -b/--run-len-bytes only sizes its bucket cells and never changes the
 * result; lengths here are full-width, so there is no b parameter. */
int grlbwt_induce_level(grlbwt_ctx *ctx, int *level, grlbwt_level_info *info);
/* exact_algo::ind_phase<b> (exact_ind_phase.cpp:674-697): parse2bwt + every level + .rl_bwt image */
int grlbwt_induce_phase(grlbwt_ctx *ctx);
int grlbwt_level_info_get(const grlbwt_ctx *ctx, int level, grlbwt_level_info *info);

/* ---- whole path: grl_bwt_algo<sym_type,false> (include/grl_bwt.hpp:23-79) -- */
int grlbwt_build(grlbwt_ctx *ctx);   /* parse_phase + induce_phase on the loaded text */

/* ---- output: replaces bwt_buff_writer + rename(bwt_lev_0 -> o_file)
 * (include/bwt_io.h:174-568, include/grl_bwt.hpp:77) ------------------------- */
int grlbwt_result_size(const grlbwt_ctx *ctx, uint64_t *image_bytes, uint64_t *n_runs);
/* device pointer of the .rl_bwt image (16-byte header + records), valid until reset/destroy */
int grlbwt_result_device_ptr(const grlbwt_ctx *ctx, const void **dev_ptr);
int grlbwt_result_download(const grlbwt_ctx *ctx, void *host_out, uint64_t capacity);
/* (pinned double-buffered download, the file is written while the next chunk comes down) */
int grlbwt_result_write_file(const grlbwt_ctx *ctx, const char *path);
/* What this context holds of the image: all of it -- (0, image_bytes) -- after grlbwt_build and grlbwt_dist_build, or this
 * rank's part after a grlbwt_dist_build with GRLBWT_COMM_KEEP_PARTS (bytes may be 0 on a rank whose slice merged into a
 * neighbour's run). */
int grlbwt_result_part(const grlbwt_ctx *ctx, uint64_t *offset, uint64_t *bytes);
/* The part at its offset of `path` (created if missing; the rank whose part ends the image sets the file's size, so a longer
 * file that was there before keeps no tail).  The file is a valid image only once EVERY rank has returned GRLBWT_OK: the caller
 * writes to a temporary name and publishes the complete file -- a barrier and a rename -- as the grlbwt executable's --gpus does. */
int grlbwt_result_write_part(const grlbwt_ctx *ctx, const char *path);

/* ---- .rl_bwt consumers: scripts/grl2plain.cpp (expand the runs) + scripts/reverse_bwt.cpp with
 * scripts/fm_index.h:79-83 (LF walk), on the device.  Rebuilds the collection (strings in input order,
 * cell_bytes-wide cells) from an .rl_bwt image in device memory into dev_text_out; used as the
 * encode -> decode round-trip check at full benchmark sizes.  64-bit positions are used when
 * the image describes >= 2^32 - 256 symbols (pass n_hint = 0 if unknown: decided from the file size). */
int grlbwt_invert_image(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes,
                        void *dev_text_out, uint64_t capacity_cells, uint64_t *n_cells_out);

/* The same LF walk (scripts/reverse_bwt.cpp:36-52), stopped after tail_cells steps per string: slot i of dev_out (tail_cells cells wide)
 * receives the LAST min(length, tail_cells) cells of string i, separator included, right-aligned; the cells in front of them are
 * left as they were.  *n_strings_out = strings, *n_cells_out = cells written.  COST: one lane per string, tail_cells dependent
 * steps each.  It was made for collections whose strings grlbwt_invert_image cannot walk end to end in a test's time (100 strings
 * of 249 M cells: 249 M dependent steps each): the ends of all strings check the ORDER of the BWT, which a symbol-count comparison
 * does not.  The whole of such a collection comes back through grlbwt_invert_image_checkpointed below, whose walks are cut into
 * segments.  capacity_cells >= strings * tail_cells. */
int grlbwt_invert_image_tails(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes, uint64_t tail_cells,
                              void *dev_out, uint64_t capacity_cells, uint64_t *n_strings_out, uint64_t *n_cells_out);

/* ---- checkpointed LF walks: the inversion and the locate index for collections of LONG strings.  The walks above run one lane per
 * string, one dependent step per cell.  Here they are cut at checkpoint rows: rows [0, n_strings) and one row, picked by a fixed
 * mixer, in every block of 2^sample_bits rows -- n_checkpoints = n_strings + ceil(n_syms / 2^sample_bits) segments of about
 * 2^sample_bits steps each, walked by lanes that take the next segment when they finish one, and put back in order by a list
 * ranking over the checkpoints.  sample_bits: 1..20, 0 = the default (8); anything else is GRLBWT_EINVAL.
 * grlbwt_invert_image_checkpointed writes byte for byte what grlbwt_invert_image writes, accepts the same images and refuses the
 * same ones with the same codes (in 32-bit positions also GRLBWT_ERANGE for 2^32 - 2 checkpoints or more).  It always takes the
 * run-indexed form; its scratch -- six words of the position width per checkpoint, three per string -- is released before it returns. */
typedef struct grlbwt_walk_info {
    uint64_t n_strings, n_checkpoints, sample_bits;   /* m = n_strings + ceil(n_syms / 2^sample_bits) */
    uint64_t longest_segment, longest_chain;          /* LF steps; checkpoints on one string's chain */
    uint64_t jump_rounds;                             /* pointer-jumping rounds run */
    uint64_t walk_lanes, lane_refills;                /* of the last walk launch */
    uint64_t scratch_bytes, sample_bytes;             /* peak scratch; bytes kept in an index (0 for the inverter) */
} grlbwt_walk_info;
int grlbwt_invert_image_checkpointed(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes,
                                     int sample_bits, void *dev_text_out, uint64_t capacity_cells,
                                     uint64_t *n_cells_out, grlbwt_walk_info *info /* may be NULL */);

/* Accepted input of every consumer (grlbwt_invert_image, _tails and _checkpointed above included): ANY well-formed image, not only
 * what grlbwt_build writes -- header widths of 1..8 bytes each, records of length 0 (they contribute nothing, as in the
 * reference's reader; grlbwt_image_split_runs writes such records itself), neighbouring records with the same symbol, run
 * lengths and totals of 2^32 and more.  An image without any record (16 bytes) is legal for plain, rle and split_runs
 * (no output symbols / runs; a 16-byte image); bwt_stats refuses it with GRLBWT_EINVAL.  The inverters need a BWT, i.e.
 * at least the separators.  Symbols are read as 64 bits: a symbol of 2^32 is not the null character of grl2plain, and
 * split_runs refuses symbols of 2^32 and more with GRLBWT_EINVAL.
 *
 * The other .rl_bwt consumers of the reference's scripts/ (SURVEY 8f-2), on an image in device memory:
 * grl2plain  (scripts/grl2plain.cpp:18-50): plain BWT, one byte per symbol ((char)sym); null_char >= 0 replaces
 *            symbol 0, -1 leaves it.
 * grlbwt2rle (scripts/grlbwt2rle.cpp:17-33): run symbols as uint8 and run lengths as uint32.
 * bwt_stats  (scripts/bwt_stats.cpp:18-98): run statistics of a byte-alphabet image; sigma reproduces the script's
 *            count (table entries whose low byte is non-zero, :57-62); decile indices past the end are clamped. */
typedef struct grlbwt_image_stats {
    uint64_t n_runs, sigma, text_size, min_run, max_run;
    uint64_t fit1, fit2, fit3;            /* runs whose length fits 1 byte / 2 bytes / needs 3 or more */
    uint64_t runs_of[256], freq_of[256];  /* per symbol: number of runs, total length */
    uint64_t deciles[9];                  /* sorted run lengths at ceil(n_runs * k/10), k = 1..9 */
    uint64_t non_maximal;                 /* runs with the same symbol as the run before them (0 for a grlBWT output) */
} grlbwt_image_stats;
int grlbwt_image_plain(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, void *dev_out_u8,
                       uint64_t capacity, int null_char, uint64_t *n_out);
int grlbwt_image_rle(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, void *dev_syms_u8, void *dev_lens_u32,
                     uint64_t capacity_runs, uint64_t *n_runs_out);
int grlbwt_image_stats_get(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, grlbwt_image_stats *out);
/* split_runs (scripts/split_runs.cpp:44-125; its argv order is `file.rlbwt bits n output_file`): re-encode the image so
 * that no run is longer than 2^bits - 1 and, for block_size > 0, no run crosses a multiple of block_size; the output is
 * an .rl_bwt image with the input's symbol width and ceil(bits/8) length bytes, byte-identical to the reference's output
 * file -- including the zero-length record the reference emits in front of a non-empty piece that starts exactly on a
 * block boundary (:87-90); an empty input record stays one empty record wherever it lies.  block_size 0 = no partition
 * (the reference asserts on it).  1 <= bits <= 63.
 * dev_out needs 16 + runs_after * (sb + ceil(bits/8)) bytes; runs_after = runs + overflow_splits + block_splits. */
typedef struct grlbwt_split_info {
    uint64_t runs_before, runs_after;     /* "Number of runs before" / "Number of runs now" */
    uint64_t overflow_splits, block_splits;
    uint64_t n_syms, n_blocks;            /* symbols described; "Number of blocks" = ceil(n_syms / block_size) */
    uint64_t out_bytes;
} grlbwt_split_info;
int grlbwt_image_split_runs(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int bits, uint64_t block_size,
                            void *dev_out, uint64_t capacity_bytes, grlbwt_split_info *info);

/* ---- counting and locating patterns in an image: one step past the reference's scripts/fm_index.h, which stops at lf().
 * grlbwt_fm_create makes an index from ANY well-formed image in device memory (see "Accepted input" above; an image without a
 * record is refused with GRLBWT_EINVAL).  The index copies what it needs -- the image may be freed when the call returns --
 * into buffers of the context's pool: two words per non-empty record, (symbol, start position) in (symbol, position) order
 * and the symbols in front of it in that order (8 + 4 bytes while the image describes fewer than 2^32 - 256 symbols, 16 + 8
 * from there on or with GRLBWT_FLAG_FORCE_IDX64).  grlbwt_fm_destroy releases it; grlbwt_ctx_destroy releases every index
 * still alive, whose handles are dead from then on.
 *
 * grlbwt_fm_count: n_patterns patterns, pattern i = cells [dev_offsets[i], dev_offsets[i + 1]) of dev_cells (cell_bytes in
 * {1, 2, 4, 8}, whatever the image's symbol width; n_patterns + 1 non-decreasing offsets).  [dev_lo[i], dev_hi[i]) are the
 * rows of the BWT whose suffixes start with the pattern -- hi - lo occurrences; lo = hi = 0 when there is none, [0, n_syms)
 * for a pattern without cells.  A cell that is no symbol of the image (a value too wide for it included) matches nothing.
 * THE SEPARATOR (the image's smallest symbol) may be a pattern's LAST cell only: there it anchors the match at the end of a
 * string.  In a BCR BWT the suffix that starts at a separator is that separator alone, ordered by the string's number, so
 * the rows of "separator, then X" are no range; a pattern with the separator anywhere else fails the WHOLE call with
 * GRLBWT_EINVAL (the message names the first such pattern; nothing is written).  One lane per pattern, a binary search over
 * the records per cell and range end; the first GRLBWT_FM_TOP_BITS (environment, 0..12, read by grlbwt_fm_create) levels
 * of every search are read from a copy in LDS.
 *
 * grlbwt_fm_locate (needs GRLBWT_FM_LOCATE): for every row of dev_rows (each < n_syms, else GRLBWT_EINVAL) the string, by
 * its number in input order, and the offset inside it at which the row's suffix starts.  COST: one dependent LF step per
 * cell between the occurrence and the START of its string -- the per-string cost model of grlbwt_invert_image_tails: fine
 * for read-like collections (strings of a few hundred cells).  For a collection of chromosomes make the index with
 * GRLBWT_FM_LOCATE | GRLBWT_FM_CHECKPOINTS: its walks end at the next checkpoint row, within about 2^sample_bits steps, and
 * making it walks segments instead of whole strings.  The walk of a row stops
 * after min(max_steps, n_syms) steps (UINT64_MAX: no cap of the caller's): an occurrence at offset o is resolved exactly when
 * o <= max_steps, an unresolved row gets UINT64_MAX in both outputs.
 * GRLBWT_FM_LOCATE adds to the index the run-start bit-vector with its ranks (a quarter byte per symbol), one LF record
 * per run and one word per string -- the number of the string behind every separator of the BWT, found by one walk over
 * every string when the index is made (the separators of a BCR BWT are ordered by the strings' contents, not by their
 * numbers).  An image whose walks do not end (not the BWT of a collection), or whose structures would take more than half
 * of the free device memory, is refused with GRLBWT_EINVAL when this flag is given, and accepted without it.
 *
 * GRLBWT_FM_CHECKPOINTS (with GRLBWT_FM_LOCATE; alone: GRLBWT_EINVAL) keeps, per checkpoint row of the walks above, the (string,
 * offset) of that row's suffix -- two words of the position width each, counted in index_bytes and in the budget -- and finds
 * the strings behind the separators from the ranked segments instead of by a walk over every string.  GRLBWT_FM_SAMPLE_BITS(b)
 * in fm_flags sets sample_bits (0 or 1..20; a value without GRLBWT_FM_CHECKPOINTS, or above 20: GRLBWT_EINVAL, *out = NULL).  grlbwt_fm_locate on such an index stops at a checkpoint row as well as at a separator; its
 * contract and its outputs are those of the index without checkpoints for every row and every max_steps (an answer found through
 * a sample whose offset is above max_steps is suppressed).  grlbwt_fm_walk_info_get: GRLBWT_EINVAL for an index without checkpoints.
 *
 * GRLBWT_FM_EXTRACT (with GRLBWT_FM_LOCATE; alone: GRLBWT_EINVAL, *out = NULL; with or without GRLBWT_FM_CHECKPOINTS) makes the index
 * a self-index: grlbwt_fm_extract returns cells of the text, which need not be kept.  COORDINATES, those of grlbwt_fm_locate:
 * string s has slen[s] cells, its separator included as the last one (offset slen[s] - 1; grlbwt_fm_string_lengths writes the
 * n_strings values of slen).  The index keeps T, the k + 1 scanned lengths, and the INVERSE of its samples: the absolute position
 * T[string] + offset of every sample, ascending, with its checkpoint beside it -- two words of the position width per sample
 * (n_samples: with checkpoints every checkpoint that lies on a string, at most n_checkpoints; without, the n_strings separators'
 * rows).  extract_bytes = (2 n_samples + n_strings + 1) position words; it is counted in index_bytes and in the budget of
 * GRLBWT_FM_LOCATE.  An index made without the bit holds what it held before, byte for byte.
 *
 * grlbwt_fm_extract: range i is cells [dev_begin[i], min(dev_end[i], slen)) of string dev_string[i] -- Python's slice rules: an
 * end of UINT64_MAX means "to the end of the string", the separator is included when the range reaches it, begin at or behind the
 * clamped end is an empty range.  The ranges go out back to back in input order as cells of cell_bytes (wide symbols as their
 * values): dev_out_offsets[i] is the first cell of range i in dev_out, dev_out_offsets[n_ranges] = *n_cells_out.  n_ranges = 0
 * is legal and writes dev_out_offsets[0] = 0.  The results are complete when the call returns.  The WHOLE call fails with
 * GRLBWT_EINVAL, and neither output buffer is written, when a dev_string[i] >= n_strings (the message names the first such
 * range), the ranges hold more than capacity_cells cells, cell_bytes is not in {1, 2, 4, 8}, the index's largest symbol does not
 * fit cell_bytes, or the index was made without GRLBWT_FM_EXTRACT.
 * COST: a range is cut at the samples inside it into pieces that are walked in parallel, each backwards from its sample's row, at
 * most the gap between neighbouring samples (with checkpoints about 2^sample_bits, at most longest_segment) dependent LF steps;
 * only the topmost piece first steps down from the sample above the range's end without writing.  Without checkpoints the only
 * samples are the strings' ends: a range costs the steps from its string's END to its begin, one lane per range -- fine for
 * read-like collections.  grlbwt_fm_extract_info_get: the counters of the last grlbwt_fm_extract on the index (GRLBWT_EINVAL for
 * an index without the bit). */
typedef struct grlbwt_fm grlbwt_fm;
#define GRLBWT_FM_LOCATE 1u      /* also build what grlbwt_fm_locate needs (one LF walk over every string, like the inverter's length pass) */
typedef struct grlbwt_fm_info {
    uint64_t n_syms, n_runs, n_strings;   /* symbols described, records kept (non-empty), occurrences of the separator */
    uint64_t sigma, separator;            /* distinct symbols, value of the smallest one */
    uint64_t idx_bytes, index_bytes;      /* 4 or 8; device bytes the index holds */
    uint64_t top_entries, flags;          /* entries of the LDS top level (0: none), fm_flags as given */
} grlbwt_fm_info;
#define GRLBWT_FM_CHECKPOINTS 2u                        /* with GRLBWT_FM_LOCATE; alone: GRLBWT_EINVAL */
#define GRLBWT_FM_SAMPLE_BITS(b) ((uint32_t)(b) << 8)   /* in fm_flags; 0 = default */
int grlbwt_fm_create(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, uint32_t fm_flags, grlbwt_fm **out);
int grlbwt_fm_destroy(grlbwt_ctx *ctx, grlbwt_fm *fm);
int grlbwt_fm_info_get(const grlbwt_fm *fm, grlbwt_fm_info *out);
int grlbwt_fm_walk_info_get(const grlbwt_fm *fm, grlbwt_walk_info *out);
int grlbwt_fm_count(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                    uint64_t n_patterns, uint64_t *dev_lo, uint64_t *dev_hi);
int grlbwt_fm_locate(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_rows, uint64_t n_rows, uint64_t max_steps,
                     uint64_t *dev_string, uint64_t *dev_offset);
#define GRLBWT_FM_EXTRACT 4u    /* with GRLBWT_FM_LOCATE; alone: GRLBWT_EINVAL. With or without GRLBWT_FM_CHECKPOINTS */
typedef struct grlbwt_fm_extract_info {
    uint64_t n_ranges, n_pieces, n_cells;   /* of the last grlbwt_fm_extract on this index */
    uint64_t walk_steps;                     /* LF steps planned: skipped + written */
    uint64_t walk_lanes, lane_refills;       /* of the walk launch, as in grlbwt_walk_info */
    uint64_t n_samples, extract_bytes;       /* entries of the inverse table; bytes GRLBWT_FM_EXTRACT added to the index */
} grlbwt_fm_extract_info;
int grlbwt_fm_string_lengths(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t *dev_len /* n_strings words, separator included */);
int grlbwt_fm_extract(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_string, const uint64_t *dev_begin, const uint64_t *dev_end,
                      uint64_t n_ranges, int cell_bytes, void *dev_out, uint64_t capacity_cells,
                      uint64_t *dev_out_offsets /* n_ranges + 1 words, written */, uint64_t *n_cells_out);
int grlbwt_fm_extract_info_get(const grlbwt_fm *fm, grlbwt_fm_extract_info *out);

/* ---- longest matches and maximal exact matches of query batches: what grlbwt_fm_count cannot say about a query that does not
 * occur whole (a read with one error, a read across two source strings, a query with an unknown base).  Both calls work on any
 * index of grlbwt_fm_create, with or without GRLBWT_FM_LOCATE, and take their patterns exactly as grlbwt_fm_count does: pattern
 * i = cells [dev_offsets[i], dev_offsets[i + 1]) of dev_cells, cell_bytes in {1, 2, 4, 8}, n_patterns + 1 non-decreasing offsets.
 * x0 = dev_offsets[0], x1 = dev_offsets[n_patterns], n_cells = x1 - x0; n_patterns = 0 and n_cells = 0 are legal and write nothing.
 *
 * grlbwt_fm_match: for cell x at offset e inside its pattern q, dev_len[x - x0] is the largest L <= e + 1 (and <= max_len when
 * max_len is not 0) such that q[e + 1 - L .. e + 1) occurs inside one string of the collection -- the backward matching
 * statistics.  A cell that is no symbol of the image gets L = 0, and so does a cell equal to THE SEPARATOR: no match holds or
 * crosses one.  Unlike grlbwt_fm_count, the separator does not anchor a match at a string's end here, and it does not fail the
 * call.  dev_lo and dev_hi are both given or both NULL (one without the other: GRLBWT_EINVAL); for L > 0 they receive the rows
 * grlbwt_fm_count returns for that substring, for L = 0 they receive 0, 0.
 *
 * grlbwt_fm_mems: the same lengths, capped by max_len in the same way.  End e of pattern i is reported when L[e] >= max(min_len, 1)
 * and e is the pattern's last cell or L[e + 1] <= L[e].  (L[e + 1] <= L[e] + 1 always, with equality exactly when the match
 * extends to the right; every length is left-maximal by definition, so without a cap the entries are exactly the maximal exact
 * matches.)  Entry j is (dev_pattern[j], dev_begin[j] = e + 1 - L, dev_mlen[j] = L, dev_lo[j], dev_hi[j]), in ascending
 * (pattern, end) order.  WITH A CAP a match of max_len cells may extend further to the left, and it is reported at every end
 * that reaches the cap.  *n_mems_out is always set; when there are more entries than `capacity`, the call fails with
 * GRLBWT_EINVAL and writes none of the output arrays (the sizing idiom of grlbwt_alphabet_compact_device: call with capacity 0).
 *
 * Both refuse with GRLBWT_EINVAL, before the first store into any output: a cell_bytes not in {1, 2, 4, 8}, decreasing offsets,
 * dev_cells missing while n_cells > 0, a null index.  GRLBWT_ENOMEM when the scratch does not fit: none for grlbwt_fm_match;
 * for grlbwt_fm_mems one word per cell for the lengths, two more when the rows are asked for, and a quarter byte per cell for
 * the flags and their ranks.
 * COST: one backward step (grlbwt_fm_count's: two binary searches over the records, the first GRLBWT_FM_TOP_BITS levels in LDS)
 * per matched cell and one more per cell, matched_cells + n_cells steps in all.  A query that lies in the collection whole costs,
 * uncapped, a number of steps quadratic in its length: max_len is what bounds it.  Fine for reads, hopeless for uncapped
 * chromosome-length queries.  One ticket per cell: lanes whose match has ended take the next cell (GRLBWT_WALK_LANES as for the
 * checkpointed walks); GRLBWT_FM_MATCH=l runs one lane per cell without refilling, with the same outputs.
 * grlbwt_fm_match_info_get: the counters of the last of the two calls that succeeded on the index. */
typedef struct grlbwt_fm_match_info {
    uint64_t n_patterns, n_cells;          /* of the last grlbwt_fm_match / grlbwt_fm_mems on this index */
    uint64_t matched_cells, longest;       /* sum and maximum of the lengths written */
    uint64_t n_capped;                     /* ends whose length is max_len (0 without a cap) */
    uint64_t n_mems;                       /* 0 after grlbwt_fm_match */
    uint64_t walk_lanes, lane_refills;     /* of the search launch, as in grlbwt_walk_info */
} grlbwt_fm_match_info;
int grlbwt_fm_match(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                    uint64_t n_patterns, uint64_t max_len /* 0: no cap */, uint64_t *dev_len /* n_cells words */,
                    uint64_t *dev_lo /* may be NULL */, uint64_t *dev_hi /* may be NULL */);
int grlbwt_fm_mems(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                   uint64_t n_patterns, uint64_t min_len, uint64_t max_len /* 0: no cap */, uint64_t *dev_pattern, uint64_t *dev_begin,
                   uint64_t *dev_mlen, uint64_t *dev_lo /* may be NULL */, uint64_t *dev_hi /* may be NULL */, uint64_t capacity,
                   uint64_t *n_mems_out);
int grlbwt_fm_match_info_get(const grlbwt_fm *fm, grlbwt_fm_match_info *out);

/* ---- patterns with up to three substituted cells: every occurrence within Hamming distance k = max_mismatches of a pattern, as
 * row ranges that feed grlbwt_fm_locate -- the backtracking search of the short-read aligners, for a read with a sequencing error
 * or a query with an unknown base.  The call works on any index, with or without GRLBWT_FM_LOCATE, and takes its patterns exactly
 * as grlbwt_fm_count and grlbwt_fm_match do (cell_bytes in {1, 2, 4, 8} whatever the image's width, n_patterns + 1 non-decreasing
 * offsets, dev_offsets[0] may be above 0, compacted alphabets are searched on their ranks).
 *
 * A HIT of pattern q (m cells) is a string v of m cells that holds no separator, differs from q at no more than k offsets and
 * occurs in the collection.  A cell of q that is no symbol of the image (a value too wide for it included), or that equals the
 * separator, can only be matched by a substitution and costs one unit of the budget; a substitute is any symbol of the image
 * except the separator and the pattern's own cell.  Different hits of one pattern have disjoint row ranges (LF is a permutation),
 * so a hit is (number of substitutions, [lo, hi), where and what was substituted); its rows are what grlbwt_fm_count answers
 * for v.  A pattern without cells has one hit, 0 substitutions and [0, n_syms); a pattern whose forced substitutions exceed k has
 * none.  Unlike grlbwt_fm_count, and like grlbwt_fm_match, the separator never anchors a match and never fails the call.
 *
 * ORDER, part of the contract: the search runs from the last cell to the first; at a cell it first tries, while budget is left,
 * every other non-separator symbol in ascending order and then the pattern's own cell.  For two hits u != v of one pattern, with
 * x the largest offset where they differ: if one of them equals q[x] there, the other one comes first; otherwise the one with the
 * smaller symbol at x.  max_hits (0: no cap) cuts each pattern's list after its first max_hits hits in this order; the
 * pattern's search ends at the next hit it meets, which is what tells a cut list (n_truncated) from one of exactly max_hits.
 * OUT OF SCOPE: choosing the best stratum only (all hits with up to k substitutions are reported, not just those with the
 * fewest), and insertions or deletions.
 *
 * OUTPUT: the hits of pattern i are entries [dev_hit_offsets[i], dev_hit_offsets[i + 1]), back to back in pattern order;
 * dev_hit_offsets[n_patterns] = *n_hits_out.  Entry j is (dev_mism[j], dev_lo[j], dev_hi[j]).  dev_sub_pos and dev_sub_val are
 * given both or neither (one alone: GRLBWT_EINVAL); when given, entry j owns max_mismatches words of each, [j * k, (j + 1) * k):
 * the substituted offsets inside the pattern in descending order and the substitute's value there (wide symbols as their
 * values); unused slots hold UINT64_MAX.  *n_hits_out is always set once the count is known; with more hits than `capacity` the
 * call fails with GRLBWT_EINVAL and writes no output array, dev_hit_offsets included (the sizing idiom of grlbwt_fm_mems: call
 * with capacity 0 and no arrays).  GRLBWT_EINVAL before the first store: max_mismatches > 3, a cell_bytes not in {1, 2, 4, 8},
 * decreasing offsets, dev_cells missing while there are cells, dev_hit_offsets missing while n_patterns > 0, hits without
 * dev_mism / dev_lo / dev_hi, a null index.  GRLBWT_ENOMEM when the scratch, one word per pattern for the counts, does not fit.
 * COST: the search runs twice, to count and to emit.  A backward step is grlbwt_fm_count's.  A cell at which a substitution
 * is open costs sigma - 2 steps, each with one more search for the next symbol present (no table of the symbols is kept, the
 * index holds what it held); the worst case grows like (m * sigma)^k / k!, pruned wherever a range empties.  Fine for DNA-like
 * alphabets and reads; slow for large alphabets at k >= 2.  max_hits bounds the output, not the pruned tree.  One ticket per
 * pattern: lanes whose search has ended take the next pattern (GRLBWT_WALK_LANES as for grlbwt_fm_match); GRLBWT_FM_MATCH=l runs
 * one lane per pattern without refilling, with the same outputs; GRLBWT_FM_TOP_BITS as for grlbwt_fm_count.
 * grlbwt_fm_approx_info_get: the counters of the last grlbwt_fm_approx that succeeded on the index. */
#define GRLBWT_FM_APPROX_MAX_K 3
typedef struct grlbwt_fm_approx_info {
    uint64_t n_patterns, n_cells, max_mismatches, max_hits;   /* of the last grlbwt_fm_approx on this index */
    uint64_t n_hits, hits_by_mismatches[4];
    uint64_t n_truncated;              /* patterns cut at max_hits */
    uint64_t steps;                    /* backward steps of the emitting pass */
    uint64_t walk_lanes, lane_refills; /* of the emitting launch, as in grlbwt_walk_info */
    uint64_t table_bytes;              /* 0 when no symbol table is kept: always, in this form */
} grlbwt_fm_approx_info;
int grlbwt_fm_approx(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                     uint64_t n_patterns, uint32_t max_mismatches, uint64_t max_hits /* per pattern; 0: no cap */,
                     uint64_t *dev_hit_offsets /* n_patterns + 1 words */, uint64_t *dev_mism, uint64_t *dev_lo, uint64_t *dev_hi,
                     uint64_t *dev_sub_pos /* may be NULL */, uint64_t *dev_sub_val /* may be NULL */, uint64_t capacity,
                     uint64_t *n_hits_out);
int grlbwt_fm_approx_info_get(const grlbwt_fm *fm, grlbwt_fm_approx_info *out);

/* ---- suffix-prefix overlaps: which strings of the collection BEGIN with a suffix of a query -- the edges of an assembly string
 * graph, what SGA-style tools build the BCR BWT of a read set for.  In a BCR BWT a string starts with w exactly when the row of
 * its whole-string suffix lies in the row range of w, and the BWT symbol of that row is the separator; the strings that start
 * with w are therefore one contiguous interval of separator ranks, [rank_sep(lo), rank_sep(hi)): one more backward step, with
 * the separator as the symbol, on the range the search already holds.  With a collection built with its reverse complements
 * (-R) the answers cover both strands.
 *
 * PREFIX RANKS: positions in the order of the whole strings as the BWT's separators hold them -- the strings sorted by their
 * cells, a string in front of every string it is a proper prefix of, equal strings by their number, empty strings first.  This
 * is the index of the table grlbwt_fm_overlap_targets reads.
 *
 * grlbwt_fm_overlaps: queries given as cells, exactly as grlbwt_fm_count takes them (cell_bytes in {1, 2, 4, 8} whatever the
 * image's width, n_patterns + 1 non-decreasing offsets, dev_offsets[0] may be above 0, compacted alphabets are searched on their
 * ranks).  It works on any index, with or without GRLBWT_FM_LOCATE.  A HIT of pattern q (m cells) is a length L with
 * max(min_len, 1) <= L <= min(m, max_len if it is not 0) such that the last L cells of q hold no separator and no value that is
 * no symbol of the image, and at least one string of the collection starts with them.  GRLBWT_FM_OVERLAP_PROPER in `flags`
 * leaves out L = m (proper suffixes only); any other flag bit is GRLBWT_EINVAL.  A string EQUAL to the suffix lies in the range:
 * without PROPER a query that is a string of the collection finds itself at L = m.  The separator and non-symbols never fail the
 * call; they end the pattern's search, since every longer suffix would hold them.
 * OUTPUT: the hits of pattern i are entries [dev_hit_offsets[i], dev_hit_offsets[i + 1]), back to back in pattern order and,
 * part of the contract, in ASCENDING L, the order the search meets them; dev_hit_offsets[n_patterns] = *n_hits_out.  Entry j is
 * (dev_len[j] = L, prefix ranks [dev_tlo[j], dev_thi[j])).  dev_lo and dev_hi are given both or neither (one alone:
 * GRLBWT_EINVAL); when given, entry j also carries the rows grlbwt_fm_count answers for that suffix.  *n_hits_out is always set
 * once the count is known; with more hits than `capacity` the call fails with GRLBWT_EINVAL and writes no output array,
 * dev_hit_offsets included (the sizing idiom of grlbwt_fm_approx: call with capacity 0 and no arrays).  GRLBWT_EINVAL before the
 * first store: unknown flag bits, one of dev_lo / dev_hi alone, a cell_bytes not in {1, 2, 4, 8}, decreasing offsets, dev_cells
 * missing while there are cells, dev_hit_offsets missing while n_patterns > 0, hits without dev_len / dev_tlo / dev_thi, a null
 * index.  GRLBWT_ENOMEM when the scratch, one word per pattern, does not fit.
 *
 * grlbwt_fm_overlaps_of: the queries are strings of the collection, by number; no text is needed beside the image.  Needs
 * GRLBWT_FM_LOCATE (without it: GRLBWT_EINVAL).  The cells of string dev_ids[i] come from the LF walk that starts at row
 * dev_ids[i], last cell first, until the separator.  Same arguments otherwise, same outputs and refusals, n_ids for n_patterns;
 * repeats are allowed; an id >= n_strings fails the whole call with GRLBWT_EINVAL before any store, the message names the first
 * such entry.  Its answers are those of grlbwt_fm_overlaps on the strings' own cells, hit for hit.
 *
 * grlbwt_fm_overlap_targets: prefix ranks to string numbers.  Needs GRLBWT_FM_LOCATE.  n_ranges pairs [dev_tlo[r], dev_thi[r]),
 * the hit columns above or any ranges; empty ranges are legal; dev_tlo[r] > dev_thi[r] or dev_thi[r] > n_strings is
 * GRLBWT_EINVAL before any store, the message names the first such range.  The entries of range r are
 * [dev_entry_offsets[r], dev_entry_offsets[r + 1]), back to back: dev_string[e] = the number of the string at prefix rank t, for
 * t ascending; dev_range (may be NULL) receives r for every entry of range r.  *n_entries_out and `capacity` follow the sizing
 * idiom (more entries than capacity: GRLBWT_EINVAL, nothing written).  2^32 ranges or more: GRLBWT_ERANGE.
 *
 * COST: one ticket per query, as grlbwt_fm_approx: the search runs from the last cell to the first, one backward step of
 * grlbwt_fm_count per cell, and from L = max(min_len, 1) on one more such step, for the separator, on a copy of the range.
 * It ends when the range empties, at a separator or non-symbol, at the query's first cell or at
 * max_len.  The search runs twice, to count and to emit.  GRLBWT_WALK_LANES, GRLBWT_FM_MATCH=l and GRLBWT_FM_TOP_BITS act as
 * for grlbwt_fm_approx.  The targets are one tile of tile_entries entries per workgroup: one search per tile, not per entry.
 * OUT OF SCOPE: transitive reduction of the overlap graph, overlaps with mismatches, prefix-suffix overlaps in the other
 * direction (build the collection with -R), a multi-GPU form, a command-line flag.
 * grlbwt_fm_overlap_info_get: the counters of the last of the three calls that succeeded on the index (the fields of the other
 * kind are 0; tile_entries is always set). */
#define GRLBWT_FM_OVERLAP_PROPER 1u
typedef struct grlbwt_fm_overlap_info {
    uint64_t n_patterns, n_cells;      /* queries; query cells the emitting pass stepped over */
    uint64_t n_hits, n_targets;        /* n_targets: the sum of dev_thi - dev_tlo over the hits */
    uint64_t longest;                  /* the largest L of a hit */
    uint64_t steps;                    /* backward steps of the emitting pass, separator steps included */
    uint64_t walk_lanes, lane_refills; /* of the emitting launch, as in grlbwt_walk_info */
    uint64_t n_ranges, n_entries;      /* of grlbwt_fm_overlap_targets */
    uint64_t tile_entries;             /* entries per workgroup of the expanding kernel */
} grlbwt_fm_overlap_info;
int grlbwt_fm_overlaps(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                       uint64_t n_patterns, uint64_t min_len /* 0: as 1 */, uint64_t max_len /* 0: no cap */, uint32_t flags,
                       uint64_t *dev_hit_offsets /* n_patterns + 1 words */, uint64_t *dev_len, uint64_t *dev_tlo, uint64_t *dev_thi,
                       uint64_t *dev_lo /* may be NULL */, uint64_t *dev_hi /* may be NULL */, uint64_t capacity, uint64_t *n_hits_out);
int grlbwt_fm_overlaps_of(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_ids, uint64_t n_ids, uint64_t min_len,
                          uint64_t max_len, uint32_t flags, uint64_t *dev_hit_offsets /* n_ids + 1 words */, uint64_t *dev_len,
                          uint64_t *dev_tlo, uint64_t *dev_thi, uint64_t *dev_lo /* may be NULL */, uint64_t *dev_hi /* may be NULL */,
                          uint64_t capacity, uint64_t *n_hits_out);
int grlbwt_fm_overlap_targets(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_tlo, const uint64_t *dev_thi, uint64_t n_ranges,
                              uint64_t *dev_entry_offsets /* n_ranges + 1 words */, uint64_t *dev_string, uint64_t *dev_range /* may be NULL */,
                              uint64_t capacity, uint64_t *n_entries_out);
int grlbwt_fm_overlap_info_get(const grlbwt_fm *fm, grlbwt_fm_overlap_info *out);

/* ---- the LCP array of the collection and its suffix-length counts: the other half of the enhanced suffix array, what BCR-style
 * tools write beside the BWT.  With it the distinct k-mer counts for every k, the nodes and edges of a de Bruijn graph and the
 * repeat structure of a read set are one pass over an array.  (Suffix / prefix overlaps are not: the array says how long an
 * overlap is, not between which strings -- grlbwt_fm_overlaps above answers that from the index.)  The call works on any index of
 * grlbwt_fm_create, with or without GRLBWT_FM_LOCATE, in both position widths and on compacted alphabets (only equality of
 * symbols matters); it makes no handle and leaves the index, its index_bytes and every later answer as they were.
 *
 * DEFINITION, part of the contract.  Rows are the rows of the BWT the image describes, in grlbwt_fm_count's coordinates: n_rows
 * of them for n_strings strings.  The suffix of row p is a run of cells followed by its string's terminator, and every
 * terminator is a symbol of its own: it equals nothing, not even another terminator.  LCP[0] = 0; for p >= 1 LCP[p] is the
 * number of leading cells the suffixes of rows p - 1 and p share.  Rows [0, n_strings) are the terminator-only suffixes and get
 * 0; two identical strings reach their full length, never more.
 *
 * VALUES: dev_lcp (may be NULL) receives n_rows values of lcp_bytes bytes, lcp_bytes in {1, 2, 4, 8}.  The effective cap is
 * min(max_lcp if it is not 0, 2^(8 * lcp_bytes) - 1); 8 bytes without max_lcp have none.  The value written is min(LCP, cap).
 * HISTOGRAMS, host arrays, each may be NULL: host_rows_at[l] = the rows whose value is exactly l (a capped row is in none),
 * host_suffixes_of[l] = the suffixes of exactly l cells = the strings of at least l cells, for l in [0, n_levels), n_levels =
 * passes + 1.  *n_levels_out is always set once the passes have run; with a histogram given and hist_capacity < n_levels the
 * call fails with GRLBWT_EINVAL and writes no output, dev_lcp included (the sizing idiom of grlbwt_fm_mems; a call whose
 * capacity may not suffice first runs its passes without storing).  Since a suffix of fewer than k cells has an LCP below k,
 * the number of distinct k-mers -- windows of k cells that hold no separator -- is the sum of host_rows_at[0, k) less the sum of
 * host_suffixes_of[0, k), for every k <= n_levels.
 *
 * ALGORITHM: B holds one bit per row, set once the row is known to differ from the row above within l cells; it starts as the
 * terminator rows and the first row of every symbol (LCP 0).  Pass l reads the rows in F-order through the runs in (symbol,
 * position) order: a row inside a run copies the bit of the row it is LF of, a run's first row tests whether B has any bit
 * between the end of the run in front and that row (a rank difference); the rows a pass adds get LCP l.  A second bit-vector,
 * the suffixes of exactly l cells, rides the same pass as a pure copy.  COST: (the largest LCP) passes, or cap - 1 if that is
 * less, each a streaming pass over the rows -- the cost model of grlbwt_merge_create: fine for read-like collections, for
 * chromosomes usable only with a cap, and a capped LCP is all that k-mer work needs.  A pass that sets no row while rows are
 * open means the image is not the BWT of a collection (the images GRLBWT_FM_LOCATE refuses for walks that do not end; e.g. the
 * records ($,1)(A,2)): GRLBWT_EINVAL.  Every well-formed image is accepted.
 * GRLBWT_EINVAL before any store: an lcp_bytes not in {1, 2, 4, 8}, a null index, all three outputs NULL.  GRLBWT_ENOMEM, before
 * the first pass, when the scratch does not fit the free memory: about 0.9 byte per row (two generations of each bit-vector, the
 * ranks of B, the F-order run-start bit-vector with its ranks).  GRLBWT_LCP_ROUND=p[lain] runs a pass through the generic
 * primitives instead of the fused kernel, with the same outputs.  OUT OF SCOPE: skipping rows that are already final, a
 * command-line flag, a multi-GPU form.
 * grlbwt_fm_lcp_info_get: the counters of the last grlbwt_fm_lcp whose passes ran on the index. */
typedef struct grlbwt_fm_lcp_info {
    uint64_t n_rows, n_strings, lcp_bytes, cap;   /* cap: the effective one (UINT64_MAX: none) */
    uint64_t passes, n_levels;                    /* n_levels = passes + 1 */
    uint64_t max_lcp, n_capped;                   /* largest value written; rows whose true LCP is >= cap */
    uint64_t tile_rows, scratch_bytes;            /* rows per workgroup of the pass kernel; peak scratch */
} grlbwt_fm_lcp_info;
int grlbwt_fm_lcp(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t max_lcp /* 0: none */, int lcp_bytes,
                  void *dev_lcp /* n_rows values, may be NULL */, uint64_t *host_rows_at /* may be NULL */,
                  uint64_t *host_suffixes_of /* may be NULL */, uint64_t hist_capacity, uint64_t *n_levels_out);
int grlbwt_fm_lcp_info_get(const grlbwt_fm *fm, grlbwt_fm_lcp_info *out);

/* ---- the document array and the generalized suffix array of the collection: the first half of the enhanced suffix array, what
 * BCR-style tools write beside the BWT and the LCP array.  For every row the string its suffix belongs to (DA) and the offset
 * inside that string (GSA): the input of document listing and counting, of coloured de Bruijn graphs on top of grlbwt_fm_lcp, of
 * string graphs on top of grlbwt_fm_overlaps, and of any tool that expects BWT + LCP + DA + SA.
 *
 * DEFINITION, part of the contract.  Rows are those of grlbwt_fm_count, coordinates those of grlbwt_fm_locate: the string by its
 * number in input order, the offset counted from the string's first cell; the separator is a string's last cell, so row
 * p < n_strings is (p, length of string p without its separator).  For p in [row_begin, row_end) entry p - row_begin of dev_string
 * and of dev_offset holds exactly what grlbwt_fm_locate writes for row p with max_steps = UINT64_MAX, narrowed to string_bytes /
 * offset_bytes bytes, each 1, 2, 4 or 8 and chosen independently; the outputs are aligned to their widths.  Either pointer may be
 * NULL (its width is then ignored); both NULL is GRLBWT_EINVAL.  row_end = UINT64_MAX means n_rows.  An empty window is legal,
 * runs no walk, writes nothing and returns GRLBWT_OK.
 * The call needs an index made with GRLBWT_FM_LOCATE (GRLBWT_EINVAL without).  The locate structures alone give form 0, one walk
 * per string; with GRLBWT_FM_CHECKPOINTS the call uses the kept samples, form 1, one walk per checkpoint segment.
 * GRLBWT_FM_EXTRACT is not required (form 0 reads the lengths from its start positions where it is there).  GRLBWT_FM_LOCATE has
 * refused an image on which a string's walk does not end; on the BWT of a collection every row lies on exactly one string's chain,
 * and on it is a checkpoint or interior to one segment, so every entry of the window is written exactly once, by one lane, without
 * atomics.  (An accepted image that is not the BWT of a collection may hold rows on no string's chain.  They have no position:
 * their entries are all bits set, grlbwt_fm_locate's UINT64_MAX narrowed.  The call sees it where the strings' lengths do not add
 * up to n_rows and fills the window before the walk.)  The call makes no handle and leaves the index, its index_bytes and every
 * later answer as they were; it works in both position widths and on compacted alphabets (only the separator's identity matters).
 *
 * GRLBWT_EINVAL before the first store, with a message that names the value: a width not in {1, 2, 4, 8} for an output that is
 * given, row_begin > row_end or row_end > n_rows, a null index, an output not aligned to its width, n_strings - 1 that does not
 * fit string_bytes, (the longest string's length without its separator) that does not fit offset_bytes.  GRLBWT_ENOMEM before the
 * first walk when the scratch does not fit the free memory: one position per walk, and one per string where form 0 writes offsets.
 *
 * COST.  A row window bounds the OUTPUT MEMORY, not the work: the rows outside it are walked and not stored.  It is there so that
 * the arrays of a collection whose 2 to 16 bytes per row do not fit beside the index can be taken in slices.  walk_steps counts
 * LF steps; a walk stops AT the row that holds the separator, so a string of L cells (separator included) takes L - 1 of them,
 * and all strings together n_rows - n_strings.  Form 1: exactly n_rows - n_strings steps (a segment that ends at the next
 * checkpoint takes the step that reaches it, a string's last segment does not step past the separator's row); the lengths and
 * their maximum come from the head samples, a reduce and no walk -- which is also what lets the call refuse before any store.
 * Form 0: n_rows - n_strings steps where the offsets need no length pass -- dev_offset is NULL, or the index was made with
 * GRLBWT_FM_EXTRACT and keeps the strings' starts -- else twice that: an index made with GRLBWT_FM_LOCATE alone keeps no
 * lengths, and a walk over every string first takes them and their maximum.  (Where such an index has rows on no chain and
 * dev_offset is NULL, the step count reveals it after the walk: the window is filled and walked a second time.)  Form 0 is one
 * dependent chain per string: fine for reads, hopeless for chromosomes.  Form 1 is the form for long strings.  Against
 * grlbwt_fm_locate over all rows -- about n_rows * (mean length) / 2 steps, with checkpoints n_rows * 2^(sample_bits - 1) --
 * both forms take one step per row.  The walks obey GRLBWT_WALK_LANES.
 * OUT OF SCOPE: the inverse suffix array, a command-line flag, a multi-GPU form, keeping the arrays inside the index (document
 * listing and counting over row ranges: grlbwt_docs_* below, a handle that keeps the document array).
 * grlbwt_fm_sa_info_get: the counters of the last grlbwt_fm_sa that succeeded on the index. */
typedef struct grlbwt_fm_sa_info {
    uint64_t n_rows, n_strings;
    uint64_t row_begin, row_end;            /* the window of the last call, end resolved */
    uint64_t string_bytes, offset_bytes;    /* 0 for an output that was not asked for */
    uint64_t n_written;                     /* row_end - row_begin */
    uint64_t form;                          /* 0: one walk per string, 1: one walk per checkpoint segment */
    uint64_t walk_steps;                    /* LF steps of all walks of the call, a length pass included */
    uint64_t longest_walk;                  /* LF steps of the longest single walk (string or segment) of the storing launch */
    uint64_t walk_lanes, lane_refills;      /* of the storing launch, as in grlbwt_walk_info */
    uint64_t scratch_bytes;
} grlbwt_fm_sa_info;
int grlbwt_fm_sa(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t row_begin, uint64_t row_end /* UINT64_MAX: n_rows */,
                 int string_bytes, void *dev_string /* may be NULL */, int offset_bytes, void *dev_offset /* may be NULL */);
int grlbwt_fm_sa_info_get(const grlbwt_fm *fm, grlbwt_fm_sa_info *out);

/* ---- the distinct k-mers of the collection with their counts, and the abundance spectrum: the table behind genome size and
 * coverage estimates, error filtering by min_count and the nodes of a de Bruijn graph -- the "one pass over the array" that
 * grlbwt_fm_lcp's comment promises, taken on the device without the array, the locate structures or a text walk per k-mer.
 *
 * DEFINITION, part of the contract.  A k-mer is a window of k cells of one string that holds no separator: the definition behind
 * grlbwt_fm_lcp's distinct counts.  The rows whose suffixes start with a given k-mer are one interval [lo, lo + count) in
 * grlbwt_fm_count's coordinates -- exactly what grlbwt_fm_count answers for the k-mer's cells -- and count is the number of the
 * k-mer's occurrences in the collection.
 *
 * THE TABLE holds the k-mers with row_begin <= lo < row_end (row_end above n_rows, UINT64_MAX for one, means n_rows) and
 * max(min_count, 1) <= count <= max_count (0: no upper bound), in ascending lo: the lexicographic order of the cells in the
 * image's symbol order.  Entry e owns dev_lo[e], dev_count[e] and the k values dev_cells[e * k .. (e + 1) * k), each cell_bytes
 * wide; wide and compacted alphabets are written as their values, as grlbwt_fm_extract writes them.  Any of the three arrays may
 * be NULL.  The window bounds the output memory, not the work, as in grlbwt_fm_sa: a partition of [0, n_rows) into windows gives
 * tables that concatenate to the whole one, and an empty window is legal.  *n_kmers_out is always set once the number is known.
 * With an array given and more entries than `capacity` the call fails with GRLBWT_EINVAL and writes nothing, the spectrum
 * included (the sizing idiom of grlbwt_fm_mems: first a call with capacity 0 and no arrays, which succeeds and reports the number).
 *
 * THE SPECTRUM: host_spectrum[c], c in [0, spectrum_bins), is the number of distinct k-mers of the WHOLE collection that occur
 * exactly c times; it ignores the window and the count filter.  The last bin collects every count >= spectrum_bins - 1; bin 0 is
 * 0 unless it is the last one (spectrum_bins = 1: bin 0 is the number of distinct k-mers).  The sum over all bins is
 * grlbwt_fm_lcp's number of distinct k-mers; info.n_windows, the sum of all counts, is the number of windows of k cells in the
 * strings: the sum over the strings of max(0, cells - k + 1).
 *
 * ALGORITHM: the passes of grlbwt_fm_lcp capped at k, without values, leave B = the rows with LCP < k: the interval boundaries.
 * A row whose suffix has fewer than k cells is a boundary that heads no k-mer.  The passes end as soon as every row is set,
 * maybe long before pass k - 1, so the generations of the suffix-length vector are continued as copy-only passes (length_passes
 * of them, until one is empty) and OR-ed: heads = B & ~short.  A head's count is the distance to the next bit of B -- in its own
 * word, or in the next non-empty word from a list of those: no scan over the gap.  The cells are k forward steps from the head
 * row: the row lies in a sorted run j (the run-start ranks of the LCP passes), starts with run j's symbol and goes on at row
 * start[j] + (row - slf[j]).  A workgroup decodes tile_kmers entries, one per lane, stages stage_bytes of cells in LDS as
 * [entry][step] -- in chunks of steps when k * cell_bytes * tile_kmers is more -- and stores the tile's span of dev_cells with
 * consecutive lanes on consecutive addresses.  One writer per entry, no atomics.
 * COST: at most k - 1 streaming passes over the rows (grlbwt_fm_lcp's cost model), a few more over the bit-vectors, and
 * forward_steps = n_selected * k dependent steps where dev_cells is given.
 *
 * GRLBWT_EINVAL before the first store: k = 0; a cell_bytes not in {1, 2, 4, 8}; dev_cells given and a symbol value of the image
 * that does not fit cell_bytes; row_begin > row_end after the clamp; spectrum_bins of 0 or above GRLBWT_FM_KMER_MAX_BINS while
 * host_spectrum is given; every output NULL (the three arrays, the spectrum and n_kmers_out); an array not aligned to its width;
 * a null index; an image that is not the BWT of a collection (the refusal of grlbwt_fm_lcp's passes).  GRLBWT_ENOMEM, before the
 * first pass, when the scratch does not fit the free memory: about one byte per row, reported as scratch_bytes.
 * The call works on any index of grlbwt_fm_create, with or without GRLBWT_FM_LOCATE, in both position widths and on compacted
 * alphabets; it makes no handle and leaves the index, its index_bytes and every later answer as they were.  GRLBWT_LCP_ROUND keeps
 * its meaning for the passes.  OUT OF SCOPE: a command-line flag, a multi-GPU form, skipping rows that are already final in the
 * passes.  Strand-merged (canonical) k-mers: grlbwt_fm_kmers_canonical.  The edges of the de Bruijn graph and its unitigs:
 * grlbwt_debruijn_create.
 * grlbwt_fm_kmer_info_get: the counters of the last grlbwt_fm_kmers on the index that got as far as counting (a call that the
 * capacity then refuses included). */
#define GRLBWT_FM_KMER_MAX_BINS 16384
typedef struct grlbwt_fm_kmer_info {
    uint64_t k, n_rows, n_strings;
    uint64_t n_distinct, n_windows;         /* distinct k-mers of the collection; the sum of their counts */
    uint64_t n_selected;                    /* entries of the table: inside the window and the count filter */
    uint64_t largest_count;
    uint64_t passes, length_passes;         /* LCP passes run; copy-only passes of the suffix lengths behind them */
    uint64_t forward_steps;                 /* n_selected * k where dev_cells was given, else 0 */
    uint64_t tile_rows, tile_kmers;         /* rows per workgroup tile of the counting kernel; entries per workgroup of the decode */
    uint64_t stage_bytes;                   /* LDS the decode stages cells in: k * cell_bytes * tile_kmers above it goes in chunks */
    uint64_t scratch_bytes;
} grlbwt_fm_kmer_info;
int grlbwt_fm_kmers(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count /* 0: none */,
                    uint64_t row_begin, uint64_t row_end /* UINT64_MAX: n_rows */, int cell_bytes, void *dev_cells /* may be NULL */,
                    uint64_t *dev_lo /* may be NULL */, uint64_t *dev_count /* may be NULL */, uint64_t capacity,
                    uint64_t *n_kmers_out, uint64_t *host_spectrum /* may be NULL */, uint64_t spectrum_bins);
int grlbwt_fm_kmer_info_get(const grlbwt_fm *fm, grlbwt_fm_kmer_info *out);

/* ---- the strand-merged (canonical) k-mers with their counts, and their abundance spectrum.  A sequenced read comes from either
 * strand, so k-mer counters count a k-mer together with its reverse complement; this call is grlbwt_fm_kmers with that merge,
 * and it names the mate of every entry, which is what strand merging of the de Bruijn graph starts from.
 *
 * DEFINITIONS, part of the contract.  Coordinates, windows and k-mers are those of grlbwt_fm_kmers.
 *   Complement map: host_pairs holds 2 * n_pairs symbol VALUES (what grlbwt_fm_extract writes); pair (a, b) means comp(a) = b
 *     and comp(b) = a; a == b is legal and makes the symbol self-complementary (an unknown base).  host_pairs == NULL with
 *     n_pairs == 0 is the DNA default (A,T), (C,G) in upper-case bytes.  A value the image does not hold is ignored: it takes no
 *     entry of the table, and a symbol paired with it has a complement that cannot occur.  A symbol in no pair has no complement.
 *   Reverse complement: rc(x) of a k-mer x = x_0 .. x_{k-1} whose cells all have complements is comp(x_{k-1}) .. comp(x_0).  A
 *     k-mer with a cell that has no complement has no reverse complement.
 *   Class: the set {x, rc(x)} restricted to the k-mers that occur in the collection.  It has one member when rc(x) does not
 *     occur, when x has no reverse complement, or when x = rc(x) (a palindrome).
 *   Representative: the member with the smaller lo -- the lexicographically smaller one among those that occur, in the image's
 *     symbol order.  total is the sum of the members' counts.  The class's mate row is the lo of the other member; for a
 *     palindrome the entry's own lo; for a class of one that is no palindrome UINT64_MAX.
 * THE TABLE holds one entry per class, in ascending lo of the representative: dev_lo[e] and dev_count[e], the representative's
 * own rows (exactly grlbwt_fm_kmers' pair), dev_mate_lo[e], dev_total[e] and the representative's k cells
 * dev_cells[e * k .. (e + 1) * k).  [mate_lo, mate_lo + total - count) is what grlbwt_fm_count answers for the reverse complement
 * of the cells when the mate exists and is not the entry itself.  min_count / max_count filter on total; the row window filters
 * on the representative's lo, bounds the output memory and not the work, and windows that partition [0, n_rows) concatenate to
 * the whole table.  Each of the five arrays may be NULL.  The sizing idiom, the alignment rule, the cell-width refusal and
 * "nothing is written on a refusal, the spectrum included" are those of grlbwt_fm_kmers.
 * THE SPECTRUM counts the classes of the WHOLE collection by total, with the bin rules of grlbwt_fm_kmers.
 * CELLS: the representative's own.  (Another convention writes the lexicographically smaller of x and rc(x) even when only the
 * larger one occurs; the two differ only for classes of one that have a reverse complement, and mate_lo == UINT64_MAX marks
 * those.  That convention is out of scope.)
 *
 * ALGORITHM: the passes, heads and counts of grlbwt_fm_kmers.  The mate pass takes one ticket per head: the forward walk from
 * the head row yields x_0, x_1, ..., and the backward search for rc(x) consumes comp(x_0), comp(x_1), ... in that same order,
 * so the two interleave -- one forward step, one backward step on a range that starts at [0, n_rows) -- and no cell is stored.
 * The walk ends when the range is empty; when the image holds a symbol that is in no pair, the forward steps alone go on to cell
 * k - 1, because n_no_complement counts every k-mer with such a cell.  A lane that ends a walk takes the next ticket (mate_tile
 * lanes per workgroup, the search array's top level and the complement table in LDS).  A head is a representative when it has
 * no mate or one at or behind it; spectrum, selection and decode then run as in grlbwt_fm_kmers over the representatives.
 * COST: grlbwt_fm_kmers' and backward_steps backward-search steps: about n_distinct * k on a collection that holds both strands,
 * about n_distinct * log_sigma(n_rows) on one that does not.  Scratch: grlbwt_fm_kmers' and one position per distinct k-mer.
 *
 * GRLBWT_EINVAL before the first pass, with a message naming the value: those of grlbwt_fm_kmers; n_pairs > 128; host_pairs ==
 * NULL with n_pairs > 0; a value listed twice in the pairs (it would have two complements, or the pair is a repeat); the
 * separator's value in a pair.  GRLBWT_ENOMEM as grlbwt_fm_kmers, and once more after the head count when the mates do not fit.
 * The call works on any index, with or without locate structures, in both position widths, on compacted and wide alphabets.  It
 * makes no handle and leaves the index, its index_bytes and every later answer as they were, grlbwt_fm_kmer_info_get included.
 * OUT OF SCOPE: the smaller-cells convention above; strand-merged nodes and unitigs of grlbwt_debruijn_* (they start from
 * mate_lo); a command-line flag; a multi-GPU form.
 * grlbwt_fm_kmers_canonical_info_get: the counters of the last grlbwt_fm_kmers_canonical on the index that got as far as counting.
 * By definition n_distinct == 2 * n_paired + n_palindromes + n_single and the sum of all totals == n_windows. */
typedef struct grlbwt_fm_ckmer_info {
    uint64_t k, n_rows, n_strings;
    uint64_t n_distinct, n_windows;         /* distinct k-mers of the collection (grlbwt_fm_kmers' number); the sum of their counts */
    uint64_t n_selected;                    /* entries of the table: classes inside the window and the filter on total */
    uint64_t n_classes;                     /* classes of the whole collection */
    uint64_t n_paired, n_palindromes;       /* classes whose two members both occur; classes whose member is its own reverse complement */
    uint64_t n_single, n_no_complement;     /* classes of one that are no palindrome; those of them with a cell that has no complement */
    uint64_t largest_total;
    uint64_t passes, length_passes;         /* as grlbwt_fm_kmer_info */
    uint64_t mate_walks;                    /* heads that started a backward search (their first cell has a complement in the image) */
    uint64_t backward_steps, forward_steps; /* of the mate pass; of the mate pass plus n_selected * k where dev_cells was given */
    uint64_t tile_rows, tile_kmers;         /* as grlbwt_fm_kmer_info */
    uint64_t mate_tile;                     /* heads (lanes) per workgroup of the mate kernel */
    uint64_t stage_bytes, scratch_bytes;
} grlbwt_fm_ckmer_info;
int grlbwt_fm_kmers_canonical(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count /* 0: none */,
                              uint64_t row_begin, uint64_t row_end /* UINT64_MAX: n_rows */, const uint64_t *host_pairs /* NULL: DNA */,
                              uint64_t n_pairs, int cell_bytes, void *dev_cells /* may be NULL */, uint64_t *dev_lo /* may be NULL */,
                              uint64_t *dev_count /* may be NULL */, uint64_t *dev_mate_lo /* may be NULL */, uint64_t *dev_total /* may be NULL */,
                              uint64_t capacity, uint64_t *n_classes_out, uint64_t *host_spectrum /* may be NULL */, uint64_t spectrum_bins);
int grlbwt_fm_kmers_canonical_info_get(const grlbwt_fm *fm, grlbwt_fm_ckmer_info *out);

/* ---- the right-maximal and maximal repeats of the collection: which row ranges are repeats at all -- the internal nodes of
 * the generalized suffix tree, what repeat analysis, repeat masking, shared-substring questions and sequence-graph construction
 * start from.  The other "one pass over the array" that grlbwt_fm_lcp's comment promises: the textbook pass is a serial stack
 * walk over the LCP array; here it is two nearest-smaller-value searches per row.
 *
 * DEFINITIONS, part of the contract.  Rows are those of grlbwt_fm_count, LCP is that of grlbwt_fm_lcp (every terminator a
 * symbol of its own, LCP[0] = 0).  A REPEAT is a string w of len >= 1 cells, none the separator, that occurs at least twice
 * in the collection; occurrences may overlap and may lie in one string.  It is RIGHT-MAXIMAL when two occurrences are followed
 * by different cells (a string's end differs from everything, another string's end included), LEFT-MAXIMAL when two are
 * preceded by different cells (a string's start differs from everything), MAXIMAL when both.  w is right-maximal exactly when
 * its row range [lo, lo + count) is an LCP interval of value len: LCP[lo] < len, LCP[lo + count] < len or lo + count = n_rows,
 * LCP[lo + 1 .. lo + count) all >= len and one of them = len.  Its SPLIT row is the first row p in (lo, lo + count) with
 * LCP[p] = len: every right-maximal repeat has exactly one, a row is the split of at most one, so there are at most n_rows - 1.
 * It is left-maximal exactly when the BWT symbols of its rows are not all one and the same symbol other than the separator --
 * decided on symbols, not on records: an image may hold neighbouring records of one symbol.
 *
 * THE TABLE holds the right-maximal repeats with max(min_len, 1) <= len <= max_len (0: no upper bound), max(min_count, 2) <=
 * count <= max_count (0: none), row_begin <= split < row_end (row_end above n_rows, UINT64_MAX for one, means n_rows) and,
 * with GRLBWT_FM_REPEATS_MAXIMAL, left-maximal as well -- in ascending split row, the in-order of the suffix tree's internal
 * nodes.  Entry e owns dev_lo[e], dev_count[e], dev_len[e] and dev_split[e]; any of the four arrays may be NULL.  The window
 * bounds the output memory, not the work: a partition of [0, n_rows) into windows gives tables that concatenate to the whole
 * one, and an empty window is legal.  *n_repeats_out is set as soon as the number is known.  With an array given and more
 * entries than `capacity` the call fails with GRLBWT_EINVAL and writes nothing (the sizing idiom of grlbwt_fm_kmers: first a
 * call with capacity 0 and no arrays, which succeeds and reports the number).
 *
 * ALGORITHM: the passes of grlbwt_fm_lcp write V = min(LCP, cap) into scratch, cap = max_len + 1 in the narrowest of 1, 2 and
 * 4 bytes that holds it (at most max_len passes; a capped row splits nothing, and comparisons against any len <= max_len stay
 * exact), without max_len the whole values in 4 bytes, 8 from 2^32 rows on.  Over V stands a tree of minima of tree_fanout
 * consecutive entries per node, level upon level up to a single node, all levels stored by a build pass (a wave reads a node):
 * about n_rows / 63 more values.  A row p with min_len <= V[p] <= max_len is a candidate.  Backward: the nearest q < p with
 * V[q] <= V[p]; p is a split row exactly when V[q] < V[p], and then lo = q.  Forward: the nearest q > p with V[q] < V[p], or
 * n_rows: lo + count.  A search scans its own node, then climbs: at each level the siblings on its side, and descends into the
 * nearest whose minimum qualifies: at most 2 * tree_levels * tree_fanout reads, whatever the input -- one string of a single
 * symbol, whose every forward search ends at the last row, included.  A workgroup takes tile_rows = tree_fanout^2 rows, one
 * node of level 1, with the tile's values and its 64 node minima in LDS; a search that reaches the tile's edge goes on in the
 * tree in memory (far_searches counts them).  Left-maximality is a rank difference on a bit-vector that marks every
 * separator's row and the first row of every record that does not continue its predecessor's symbol: no scan of the range.
 * The selection is written as ballot words and ranked by a scan; the emit walks the set bits with every lane on a selected
 * row (the compaction of grlbwt_fm_kmers' generic decode), repeats that row's two searches in the tree in memory and stores
 * by rank -- consecutive lanes on consecutive entries, one writer per entry, no per-row scratch.  (An emit over the same tiles
 * with the values in LDS measured 1.4 to 3.4 times slower, since it walks every row of every tile that holds a selected one;
 * it is not kept.)  No thread waits for another; the only atomics set the head bits.
 * COST: the LCP passes (grlbwt_fm_lcp's cost model; max_len bounds them), one pass over V per tree level, the search pass,
 * the emit pass.  Scratch: the passes' 0.9 byte per row and value_bytes * 64 / 63 per row, reported as scratch_bytes.
 *
 * GRLBWT_EINVAL before the first store: unknown flag bits; max_len given and below max(min_len, 1); row_begin above the clamped
 * row_end; every output NULL (the four arrays and n_repeats_out); an array not aligned to 8; a null index; an image that is
 * not the BWT of a collection (the refusal of grlbwt_fm_lcp's passes).  GRLBWT_ENOMEM, before the first pass, when the scratch
 * does not fit the free memory.  The call works on any index of grlbwt_fm_create, with or without the locate structures, in
 * both position widths and on compacted and wide alphabets; it makes no handle and leaves the index, its index_bytes and every
 * later answer of every other call as they were.  GRLBWT_LCP_ROUND keeps its meaning for the passes.
 * OUT OF SCOPE: supermaximal repeats; the repeats' cells (grlbwt_fm_locate of row lo, then grlbwt_fm_extract of len cells); a
 * histogram by length; tandem repeats; a command-line flag; a multi-GPU form.
 * grlbwt_fm_repeat_info_get: the counters of the last grlbwt_fm_repeats on the index that got as far as counting (a call that
 * the capacity then refuses included). */
#define GRLBWT_FM_REPEATS_MAXIMAL 1u      /* only the repeats that are left-maximal too */
typedef struct grlbwt_fm_repeat_info {
    uint64_t n_rows, n_strings;
    uint64_t min_len, max_len;              /* the effective values: min_len at least 1, max_len 0 for none */
    uint64_t passes;                        /* LCP passes run */
    uint64_t n_repeats, n_maximal;          /* right-maximal repeats inside the length bounds, ignoring count, window and flag; the left-maximal of them */
    uint64_t n_selected;                    /* entries of the table */
    uint64_t longest, largest_count;        /* over n_repeats */
    uint64_t value_bytes;                   /* width of the values held in scratch */
    uint64_t tile_rows, tree_fanout, tree_levels;   /* rows per workgroup; entries per node; levels of the tree, the values' included */
    uint64_t far_searches;                  /* searches of the count pass, two per split row at the most, that left their tile; 0 in the generic form */
    uint64_t scratch_bytes;
} grlbwt_fm_repeat_info;
int grlbwt_fm_repeats(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t min_len, uint64_t max_len /* 0: none */, uint64_t min_count,
                      uint64_t max_count /* 0: none */, uint32_t repeat_flags, uint64_t row_begin, uint64_t row_end /* UINT64_MAX: n_rows */,
                      uint64_t *dev_lo, uint64_t *dev_count, uint64_t *dev_len, uint64_t *dev_split /* each may be NULL */,
                      uint64_t capacity, uint64_t *n_repeats_out);
int grlbwt_fm_repeat_info_get(const grlbwt_fm *fm, grlbwt_fm_repeat_info *out);

/* ---- the strings behind row ranges: document listing and counting, the question a collection index exists for -- which reads
 * carry this k-mer, which genomes of a pangenome carry this allele, what is the document frequency of a k-mer.  grlbwt_fm_count
 * says how often a pattern occurs and grlbwt_fm_locate where each occurrence lies; these calls say WHICH STRINGS hold it and how
 * many do, for batches of row ranges: the (lo, hi) pairs of grlbwt_fm_count, the (lo, lo + count) table of grlbwt_fm_kmers, or
 * any ranges.  Without them the route is one grlbwt_fm_locate per occurrence and a unique on the host.
 *
 * DEFINITIONS, part of the contract.  Rows are those of grlbwt_fm_count, strings are numbered as grlbwt_fm_locate numbers them.
 * DA[p] is the string of row p, exactly what grlbwt_fm_sa writes.  For a range [lo, hi) with lo <= hi <= n_rows its DOCUMENTS
 * are the distinct values of DA[lo .. hi); the OCCURRENCES of document d are the rows p of the range with DA[p] = d; its FIRST
 * ROW is the smallest such p.  The documents of a range are reported in ASCENDING FIRST ROW: the order of each string's smallest
 * matching suffix, and the order the filter below meets them.  An empty range has no document; (0, 0), the "no occurrence"
 * answer of grlbwt_fm_count, is legal.  Ranges may overlap, repeat and come in any order.
 *
 * grlbwt_docs_create makes a handle from an index made with GRLBWT_FM_LOCATE (without it: GRLBWT_EINVAL, the message says so).
 * It uses form 0 or form 1 of grlbwt_fm_sa's walk, whichever the index offers, computes what it keeps and holds no pointer into
 * the index afterwards: the index may be destroyed first.  grlbwt_ctx_destroy releases the handles still alive.  The handle
 * keeps, in words of the index's position width (idx_bytes):
 *   DA     one word per row;
 *   PREV   one word per row: the largest row below p with the same string, or "none";
 *   with GRLBWT_DOCS_OCCURRENCES also
 *   LST    one word per row: the rows sorted by (string, row);
 *   START  n_strings + 1 words: where each string's rows begin in LST (every string owns at least its terminator's row).
 * DA comes from the walk; a stable sort of (DA, row) on sort_bits = ceil(log2 n_strings) key bits leaves every string's rows
 * ascending (LST); PREV[LST[i]] = LST[i - 1] where both belong to one string; START from the key changes.  The sort's buffers
 * are released before the call returns.  Refusals, each with *out = NULL and nothing held: unknown flag bits, a null index
 * (GRLBWT_EINVAL); an index whose strings' lengths do not add up to n_rows -- rows on no string's chain, the case
 * grlbwt_fm_sa fills with all-ones -- GRLBWT_EINVAL, the message says that the image is not the BWT of a collection; held bytes
 * plus peak scratch (four words per row and one per walk) above the free device memory: GRLBWT_ENOMEM, before the first walk.
 * The index, its index_bytes and every later answer of it are unchanged.  Both position widths; compacted and wide alphabets
 * (only string numbers matter, not symbols).
 *
 * grlbwt_docs_count: dev_ndocs[r] = the number of documents of range r, *n_docs_total_out their sum.  n_ranges = 0 is legal,
 * writes nothing and reports 0.  It is the sizing call of grlbwt_docs_list.
 * grlbwt_docs_list: the documents of range r are entries [dev_entry_offsets[r], dev_entry_offsets[r + 1]), back to back, in the
 * contract's order; dev_entry_offsets[n_ranges] = *n_entries_out.  Entry e is dev_string[e]; dev_first_row[e], a row that
 * grlbwt_fm_locate turns into an offset; dev_occ[e], the occurrences of that document in the range; dev_range[e] = r.  The last
 * three may be NULL.  dev_occ on a handle made without GRLBWT_DOCS_OCCURRENCES is GRLBWT_EINVAL.  *n_entries_out is set whenever
 * the count was reached; more entries than `capacity` is GRLBWT_EINVAL and nothing is written (the rule of
 * grlbwt_fm_overlap_targets).  n_ranges = 0 writes dev_entry_offsets[0] = 0.
 * Refusals of both, before the first store into any output: a range with lo > hi or hi > n_rows (GRLBWT_EINVAL, the message
 * names the first such range); a null handle; a missing output -- dev_ndocs; dev_entry_offsets; dev_string while there are
 * entries -- (GRLBWT_EINVAL); 2^32 ranges or more, or more tiles than one launch takes (GRLBWT_ERANGE); scratch that does not
 * fit the free memory (GRLBWT_ENOMEM): one bit per range row for the flags, their word ranks, n_ranges + 1 words of scanned sizes.
 *
 * COST.  The create: one LF step per row and ceil(sort_bits / 8) sort passes over the rows.  A query: n_range_rows row visits,
 * one coalesced read of PREV per range row -- row p of range r is its document's first row exactly when PREV[p] is none or
 * below lo[r]; no sort and no hash per query.  A range is linear in its SIZE, not in its number of documents.  With dev_occ each
 * entry adds two binary searches in its string's part of LST.  The device form is two kernels over tiles of tile_entries range
 * rows per workgroup: one search per tile, one writer per output word, no atomics.
 * OUT OF SCOPE: sub-linear counting, top-k by occurrences, a min_occ filter, a command-line flag, a multi-GPU form.
 * grlbwt_docs_info_get: the handle, its create, and the counters of the last query that succeeded on it. */
typedef struct grlbwt_docs grlbwt_docs;
#define GRLBWT_DOCS_OCCURRENCES 1u   /* also keep what dev_occ needs */
typedef struct grlbwt_docs_info {
    uint64_t n_rows, n_strings;
    uint64_t flags;                         /* the docs_flags of the create */
    uint64_t idx_bytes, held_bytes;         /* the width of a kept word; the device memory the handle holds */
    uint64_t scratch_bytes;                 /* of the create, at its peak, beside what the handle holds */
    uint64_t sort_bits;                     /* ceil(log2 n_strings) */
    uint64_t form;                          /* 0: one walk per string, 1: one walk per checkpoint segment */
    uint64_t walk_steps;                    /* LF steps of the create */
    uint64_t n_ranges, n_range_rows;        /* of the last query that succeeded: ranges, the sum of hi - lo */
    uint64_t n_entries;                     /* documents over all ranges (grlbwt_docs_count: the total) */
    uint64_t largest_range, most_docs;      /* the largest hi - lo; the most documents of one range */
    uint64_t tile_entries;                  /* range rows per workgroup of the two kernels */
} grlbwt_docs_info;
int grlbwt_docs_create(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint32_t docs_flags, grlbwt_docs **out);
int grlbwt_docs_destroy(grlbwt_ctx *ctx, grlbwt_docs *docs);
int grlbwt_docs_info_get(const grlbwt_docs *docs, grlbwt_docs_info *out);
int grlbwt_docs_count(grlbwt_ctx *ctx, const grlbwt_docs *docs, const uint64_t *dev_lo, const uint64_t *dev_hi, uint64_t n_ranges,
                      uint64_t *dev_ndocs /* n_ranges words */, uint64_t *n_docs_total_out);
int grlbwt_docs_list(grlbwt_ctx *ctx, const grlbwt_docs *docs, const uint64_t *dev_lo, const uint64_t *dev_hi, uint64_t n_ranges,
                     uint64_t *dev_entry_offsets /* n_ranges + 1 words */, uint64_t *dev_string, uint64_t *dev_first_row /* may be NULL */,
                     uint64_t *dev_occ /* may be NULL */, uint64_t *dev_range /* may be NULL */, uint64_t capacity, uint64_t *n_entries_out);

/* ---- the compacted de Bruijn graph of the collection: the nodes that grlbwt_fm_kmers writes, the edges between them with their
 * weights, the degrees, and the unitigs (maximal non-branching paths) with their nodes and cells -- what an assembler or a
 * sequence-graph builder takes from a k-mer counter and a compactor, from the .rl_bwt image alone, on the device.
 *
 * DEFINITIONS, part of the contract.  Coordinates are those of grlbwt_fm_count and grlbwt_fm_kmers; a window is a run of cells
 * of one string that holds no separator.
 *   NODE: a distinct k-mer with max(min_count, 1) <= count <= max_count (0: no upper bound).  Node id v is the k-mer's index in
 *     the whole-window table of grlbwt_fm_kmers(k, min_count, max_count): ids 0 .. n_nodes - 1 in ascending lo, lexicographic order.
 *   EDGE u -> v: a window w of k + 1 cells that occurs in the collection, whose first k cells are node u and whose last k cells
 *     are node v.  Its weight is the number of occurrences of w, its row the lo of w: [row, row + weight) is what
 *     grlbwt_fm_count answers for w.  The graph is edge-centric: two nodes that overlap by k - 1 cells but never occur side by
 *     side have no edge; an edge whose other end was filtered out does not exist; a self-loop (AAA, k = 2) is an edge.
 *   EDGE ORDER: ascending (to, from) -- for a fixed `to` also ascending first cell of `from`.  The table is the CSR of in-edges:
 *     the in-edges of v are entries dev_in_offsets[v] .. dev_in_offsets[v + 1].
 *   DEGREES: in_degree[v] and out_degree[v] count edges of the filtered graph.
 *   UNITIG: an edge u -> v is compactable when out_degree[u] == 1 and in_degree[v] == 1.  A unitig is a maximal path
 *     v_0 .. v_{m-1} whose consecutive edges are all compactable; every node lies in exactly one unitig, which may be a single
 *     node.  A component in which every node has in-degree and out-degree 1 through compactable edges is a cycle, down to one
 *     node with a self-loop: one CIRCULAR unitig that starts at its smallest node id and does not repeat that node at its end.
 *   UNITIG ORDER: ascending id of the first node.
 *   UNITIG CELLS: unitig j of m nodes has k + m - 1 cells, the k cells of v_0 followed by the last cell of each further node.
 *     The cells of all unitigs lie back to back, those of unitig j from dev_node_offsets[j] + j * (k - 1) on: a closed form, no
 *     cell-offset array is written; n_cells = n_nodes + n_unitigs * (k - 1).  Wide and compacted alphabets are written as their
 *     values, as grlbwt_fm_extract and grlbwt_fm_kmers write them.
 *   UNITIG WEIGHT: the sum of the counts of its nodes.
 * Strands are not merged: a collection built with -R holds both strands and yields both copies of every unitig.
 *
 * grlbwt_debruijn_create does all the work; info has the exact sizes; the three writers copy and decode.  Every output array of
 * a writer is optional; a call with no array at all is GRLBWT_EINVAL, and so is an array together with a capacity below what
 * info reports (nodes: n_nodes; edges: n_edges, dev_in_offsets takes n_nodes + 1 words whatever the capacity; unitigs: n_unitigs
 * for node_offsets (+ 1 word) / weight / circular, n_nodes for dev_nodes, n_cells for dev_cells) -- nothing is written then.
 * grlbwt_debruijn_nodes: dev_unitig[v] and dev_rank[v] are v's unitig and its place inside it.  The handle holds no pointer into
 * the index, which may be destroyed first; only grlbwt_debruijn_unitigs with dev_cells reads the index again, for the forward
 * steps: it must be the index the handle was made from (checked by its sizes and a fingerprint of its runs taken at create time,
 * GRLBWT_EINVAL otherwise), and a symbol value that does not fit cell_bytes is refused before the first store.  Without dev_cells
 * the index may be NULL.
 *
 * ALGORITHM: the passes and the selection of grlbwt_fm_kmers give the nodes.  For node v with rows [lo, hi), every symbol a above
 * the separator that occurs in BWT[lo, hi) takes one backward step to [lo2, hi2), the rows of a.v -- always a window of k + 1
 * cells, because the BWT symbol of a row whose suffix starts with k cells of a string precedes them in that string.  The last
 * boundary bit at or before lo2 heads the k-mer of its first k cells; if that head is selected, this is an edge from its rank.
 * The symbols come in ascending order from the lower bound of (a + 1, 0) in the sorted runs, and the enumeration ends as soon as
 * the steps account for all of the node's rows, so a node whose rows hold one symbol stops at it.  Two passes of this one search
 * (grlbwt_fm_approx's shape): the first writes in_degree and adds to out_degree, a scan gives in_offsets, the second writes the
 * entries.  A workgroup's lanes take tile_nodes consecutive nodes under the LDS top level of the searches and store their own
 * entries, which for consecutive nodes are consecutive entries.  Unitigs: link[v] is v's only in-edge when it is
 * compactable; pointer jumping in counted rounds of separate launches, at most ceil(log2 n_nodes) + 1, carries (pointer, steps,
 * smallest id seen); what has found no head then lies on cycles, whose smallest ids become heads, and a second set of rounds
 * ranks their nodes.  Nothing waits for another thread.  The cell at place r < m of a unitig is the first cell of its r-th node,
 * read off the sorted run that holds the node's lo; the last k - 1 cells are k - 1 forward steps from the last node's lo, the
 * only dependent chains: n_unitigs * (k - 1) steps.  A workgroup writes tile_cells consecutive cells after one search per tile
 * for its unitigs, consecutive lanes on consecutive addresses.
 *
 * grlbwt_debruijn_create refuses with GRLBWT_EINVAL: k = 0; min_count > max_count != 0; flags other than 0; a null index; an
 * image that is not the BWT of a collection (the refusal of grlbwt_fm_lcp's passes); with GRLBWT_ENOMEM scratch that does not fit
 * the free memory, before the first pass.  k larger than every string and n_rows = 0 give legal empty graphs.  It works on any
 * index of grlbwt_fm_create, with or without GRLBWT_FM_LOCATE, in both position widths and on compacted alphabets, and leaves
 * the index as it was.  The context releases the handles that are still alive.
 * OUT OF SCOPE: canonical (strand-merged) nodes (grlbwt_cdebruijn_* below), a GFA writer, tip and bubble removal, a command-line flag, a multi-GPU form. */
typedef struct grlbwt_debruijn grlbwt_debruijn;
typedef struct grlbwt_debruijn_info {
    uint64_t k, n_rows, n_strings;
    uint64_t n_distinct;                  /* distinct k-mers of the collection (grlbwt_fm_kmers' number) */
    uint64_t n_nodes, n_edges;            /* after the count filter */
    uint64_t n_unitigs, n_circular, longest_unitig /* nodes */, n_cells;
    uint64_t max_in_degree, max_out_degree;
    uint64_t passes, length_passes;       /* as grlbwt_fm_kmer_info */
    uint64_t backward_steps;              /* of the edge search, both passes */
    uint64_t jump_rounds;                 /* pointer-jumping rounds run, the cycle rounds included */
    uint64_t tile_nodes, tile_cells;      /* nodes per workgroup step of the edge search; cells per workgroup of the unitig decode */
    uint64_t handle_bytes, scratch_bytes;
} grlbwt_debruijn_info;
int grlbwt_debruijn_create(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count /* 0: none */,
                           uint32_t debruijn_flags /* 0 */, grlbwt_debruijn **out);
int grlbwt_debruijn_destroy(grlbwt_ctx *ctx, grlbwt_debruijn *graph);
int grlbwt_debruijn_info_get(const grlbwt_debruijn *graph, grlbwt_debruijn_info *out);
int grlbwt_debruijn_nodes(grlbwt_ctx *ctx, const grlbwt_debruijn *graph, uint64_t *dev_lo, uint64_t *dev_count, uint32_t *dev_in_degree,
                          uint32_t *dev_out_degree, uint64_t *dev_unitig, uint64_t *dev_rank /* place inside its unitig */, uint64_t capacity);
int grlbwt_debruijn_edges(grlbwt_ctx *ctx, const grlbwt_debruijn *graph, uint64_t *dev_in_offsets /* n_nodes + 1 */, uint64_t *dev_from,
                          uint64_t *dev_weight, uint64_t *dev_row, uint64_t capacity /* edges */);
int grlbwt_debruijn_unitigs(grlbwt_ctx *ctx, const grlbwt_debruijn *graph, const grlbwt_fm *fm, int cell_bytes,
                            uint64_t *dev_node_offsets /* n_unitigs + 1 */, uint64_t *dev_nodes /* n_nodes */, void *dev_cells /* n_cells */,
                            uint64_t *dev_weight, uint8_t *dev_circular, uint64_t capacity_unitigs, uint64_t capacity_nodes,
                            uint64_t capacity_cells);

/* ---- the strand-merged (bidirected) compacted de Bruijn graph of the collection: the nodes are the classes {x, rc(x)} that
 * grlbwt_fm_kmers_canonical writes, the edges join node ENDS, and the unitigs are reported as one reading each -- the graph that
 * BCALM-style compactors write, which assemblers and sequence-graph builders take, from the .rl_bwt image alone, on the device.
 * A read set holds both strands: grlbwt_debruijn_* reports every unitig of a collection built with -R twice, and splits the graph
 * of a one-strand read set wherever the coverage changes strand; this graph does neither.
 *
 * DEFINITIONS, part of the contract.  Conventions are those of grlbwt_debruijn_* unless stated; the complement map (host_pairs,
 * n_pairs) is that of grlbwt_fm_kmers_canonical, with its refusals.
 *   NODE: node v is the v-th entry of the whole-window table of grlbwt_fm_kmers_canonical(k, min_count, max_count, pairs): ids
 *     ascend with the representative's lo; lo, count, mate_lo and total are that table's; the filter goes by total.  A node is
 *     RIGID when it is a palindrome (mate_lo == lo) or when a cell of its k-mer has no complement.
 *   ENDS: node v has end 0, in front of the representative's first cell, and end 1, behind its last cell; end id 2 v + e.  A
 *     palindrome has only end 0: everything incident to it is reported there and its end 1 stays empty.
 *   HALF-EDGES: let w be a window of k + 1 cells that occurs, p its first k cells and s its last k cells, both classes nodes.
 *     w LEAVES p's node u through end 1 when p is u's representative and through end 0 when p is the mate; w ENTERS s's node v
 *     through end 0 when s is the representative and through end 1 when s is the mate; for a palindrome both are end 0.  w gives
 *     the half-edges (u,eu) -> (v,ev) and (v,ev) -> (u,eu); rc(w), where it occurs, gives the same two.  The table has one entry
 *     per distinct (source end, other end): `other` is the other end's id; `weight` the occurrences of w plus those of rc(w);
 *     [fwd_row, fwd_row + fwd_count) is what grlbwt_fm_count answers for the window as read from the source end to the other
 *     end, UINT64_MAX and 0 when only its reverse complement occurs.  A window that is its own reverse complement gives a
 *     HAIRPIN, source end == other end, stored once with weight = fwd_count; nothing else is a hairpin.
 *     The table is the CSR over the 2 n_nodes ends in ascending (source end, other end): the half-edges of end a are entries
 *     dev_end_offsets[a] .. dev_end_offsets[a + 1]; degree0 and degree1 are the segment lengths of a node's two ends.
 *     n_half_edges = 2 n_edges - n_hairpins, and the edges' weights, each edge counted once, sum to the number of windows of
 *     k + 1 cells whose two k-mers are both nodes.
 *   UNITIGS: a half-edge a -> b is compactable when both ends have degree 1, a != b and neither node is rigid.  A rigid node is
 *     always a unitig of its own, in orientation +.  A unitig is a maximal chain over compactable half-edges; every node lies in
 *     exactly one.  It is reported as one READING: oriented nodes 2 v + o, o = 1 meaning that v is read as the reverse
 *     complement of its representative.  Normal form: a path of m >= 2 nodes takes the reading whose first node has the smaller
 *     id of the two end nodes; a single node is +; a circular unitig starts at its smallest node in orientation +, down to one
 *     node whose end 1 links to its own end 0.  Unitigs are numbered by the id of their first node.  Unitig j of m nodes spells
 *     k + m - 1 cells from dev_node_offsets[j] + j * (k - 1) on, n_cells = n_nodes + n_unitigs * (k - 1); its weight is the
 *     sum of its nodes' totals.  In the nodes call dev_orient[v] is o.  A - node whose mate does not occur is spelled through the
 *     complement VALUES of the pairs, which the image need not hold and which must fit cell_bytes like the symbols.
 *
 * grlbwt_cdebruijn_create does all the work; info has the exact sizes; the three writers copy and decode.  Every output array is
 * optional; a call with no array is GRLBWT_EINVAL, and a capacity below info's number (nodes: n_nodes; links: n_half_edges,
 * dev_end_offsets takes 2 n_nodes + 1 words whatever the capacity; unitigs: as grlbwt_debruijn_unitigs) is refused before any
 * store.  The handle holds no pointer into the index; only the cells read the index again, behind the fingerprint check.
 *
 * ALGORITHM: the passes, the mate pass and the selection of grlbwt_fm_kmers_canonical give the nodes.  The edge search of
 * grlbwt_debruijn_create runs from every head, representative or mate, whose class is selected, count then emit, and writes
 * records: a forward one (source end, other end, lo(w), occ(w)) per window and its reverse (weight only) unless it is a
 * hairpin.  Two stable sorts of the record numbers, by other end and by source end, put the at most two records of an entry side
 * by side; one pass flags the group heads as ballot words and a second stores the merged entries of a tile of records behind a
 * scan of the tile counts.  Unitigs: the doubled graph of 2 n_nodes oriented nodes, succ(v, o) = the compactable partner of end
 * 1 - o, on which every unitig appears as two disjoint chains; the counted pointer-jumping rounds of grlbwt_debruijn_create rank
 * both, and a path keeps the chain whose head node id is below its tail's, a cycle the chain whose smallest oriented id is even.
 * Cells: a tile of consecutive cells per workgroup, one search per tile; the - nodes without a mate walk k forward steps each as
 * tickets.  Nothing waits for another thread.
 *
 * grlbwt_cdebruijn_create refuses with GRLBWT_EINVAL what grlbwt_debruijn_create and the pairs of grlbwt_fm_kmers_canonical
 * refuse; with GRLBWT_ENOMEM scratch that does not fit, before the pass it belongs to; with GRLBWT_ERANGE a graph of 2^31 nodes
 * or more on a context with 32-bit positions (end ids take one more bit than node ids).  k longer than every string and n_rows = 0
 * give legal empty graphs.  Both position widths, compacted and wide alphabets; the index and the record of
 * grlbwt_fm_kmers_canonical_info_get are left as they were.  The context releases the handles that are still alive.
 * OUT OF SCOPE: unitig-level link lists and a GFA writer; spelling the smaller of x and rc(x) when only the larger occurs; tip and
 * bubble removal; compaction through rigid nodes; a command-line flag; a multi-GPU form. */
typedef struct grlbwt_cdebruijn grlbwt_cdebruijn;
typedef struct grlbwt_cdebruijn_info {
    uint64_t k, n_rows, n_strings;
    uint64_t n_distinct;                  /* distinct k-mers of the collection (grlbwt_fm_kmers' number) */
    uint64_t n_nodes, n_rigid, n_palindromes;       /* after the filter by total */
    uint64_t n_edges, n_half_edges, n_hairpins;
    uint64_t n_unitigs, n_circular, longest_unitig /* nodes */, n_cells;
    uint64_t max_end_degree;
    uint64_t passes, length_passes;       /* as grlbwt_fm_kmer_info */
    uint64_t mate_backward_steps;         /* of the mate pass */
    uint64_t edge_backward_steps;         /* of the edge search, both passes */
    uint64_t forward_steps;               /* of the create: the mate pass's */
    uint64_t cells_forward_steps;         /* of the last grlbwt_cdebruijn_unitigs that wrote cells */
    uint64_t jump_rounds;                 /* pointer-jumping rounds run on the doubled graph, the cycle rounds included */
    uint64_t tile_nodes, tile_cells;      /* heads per workgroup step of the edge search; cells per workgroup of the unitig decode */
    uint64_t handle_bytes, scratch_bytes;
} grlbwt_cdebruijn_info;
int grlbwt_cdebruijn_create(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count /* 0: none */,
                            const uint64_t *host_pairs /* NULL: DNA */, uint64_t n_pairs, uint32_t cdebruijn_flags /* 0 */, grlbwt_cdebruijn **out);
int grlbwt_cdebruijn_destroy(grlbwt_ctx *ctx, grlbwt_cdebruijn *graph);
int grlbwt_cdebruijn_info_get(const grlbwt_cdebruijn *graph, grlbwt_cdebruijn_info *out);
int grlbwt_cdebruijn_nodes(grlbwt_ctx *ctx, const grlbwt_cdebruijn *graph, uint64_t *dev_lo, uint64_t *dev_count, uint64_t *dev_mate_lo,
                           uint64_t *dev_total, uint32_t *dev_degree0, uint32_t *dev_degree1, uint64_t *dev_unitig, uint64_t *dev_rank,
                           uint8_t *dev_orient, uint64_t capacity);
int grlbwt_cdebruijn_links(grlbwt_ctx *ctx, const grlbwt_cdebruijn *graph, uint64_t *dev_end_offsets /* 2 n_nodes + 1 */, uint64_t *dev_other,
                           uint64_t *dev_weight, uint64_t *dev_fwd_row, uint64_t *dev_fwd_count, uint64_t capacity /* half-edges */);
int grlbwt_cdebruijn_unitigs(grlbwt_ctx *ctx, const grlbwt_cdebruijn *graph, const grlbwt_fm *fm, int cell_bytes,
                             uint64_t *dev_node_offsets /* n_unitigs + 1 */, uint64_t *dev_nodes /* n_nodes oriented nodes 2 v + o */,
                             void *dev_cells /* n_cells */, uint64_t *dev_weight, uint8_t *dev_circular, uint64_t capacity_unitigs,
                             uint64_t capacity_nodes, uint64_t capacity_cells);

/* ---- merging two images: the image of the collection "strings of A, then strings of B" from the images of A and B, without the
 * texts -- a collection larger than one build is built in batches and folded together, a batch of new strings is added to an
 * existing image.  String i of B becomes string n_strings_a + i.  When A and B were built by this engine with cells of cell_bytes,
 * the output is byte for byte what grlbwt_build writes for the concatenated text, header included: sb from the largest symbol of
 * both images + 4, fb from the largest total of one symbol in the merged BWT (cell_bytes 1) or from the merged length (2, 4, 8) --
 * which is why the call takes cell_bytes, as grlbwt_invert_image does.  Any well-formed image is accepted ("Accepted input"
 * above); the output always has maximal runs, no empty record and those widths.
 *
 * The algorithm is the interleave refinement of Holt and McMillan (2014) with the separator rule of the BCR order: one flag per
 * merged row (0: the row comes from A), 0^nA 1^nB to begin with; a round writes every row's flag where a stable sort of the rows
 * by their symbol puts it, then sets the separator's bucket -- the first n_strings_a + n_strings_b rows -- to 0^kA 1^kB (the
 * terminators are ordered by the strings' numbers); the rounds end with the one that changes nothing.  COST: about (the longest
 * prefix a suffix of A shares with a suffix of B) + 2 rounds, each a streaming pass over the merged rows -- the per-string cost
 * model of grlbwt_fm_locate without checkpoints: fine for read-like collections (read length + 1 rounds), hopeless for
 * chromosomes.  max_rounds bounds them (0: n + 2); a merge that has not converged by then fails with GRLBWT_EINVAL.
 * SCOPE: both images together hold at most 256 distinct symbols (a round sorts by one byte); more: GRLBWT_ERANGE.
 * Device memory: one byte per row of A and of B and one per merged row are kept in the handle (held_bytes); the rounds take a
 * second byte per merged row and tile tables on top (scratch_bytes), checked against the free memory before the first round
 * (GRLBWT_ENOMEM).  64-bit positions from 2^32 - 256 merged rows on or with GRLBWT_FLAG_FORCE_IDX64; 2^40 rows or more:
 * GRLBWT_ERANGE.  GRLBWT_EINVAL: an image without a record or with a bad header, cell_bytes not in {1, 2, 4, 8}, a symbol that
 * does not fit cell_bytes, images whose smallest symbols differ (the message names both), capacity_bytes < out_bytes.  On failure
 * *out = NULL and nothing is written.
 * grlbwt_merge_create copies what it needs -- both images may be freed when it returns -- and runs all rounds; grlbwt_merge_emit
 * writes the merged image (out_bytes of the info); grlbwt_merge_interleave the converged interleave as ceil(n / 64) words, bit p
 * of word p / 64 set when row p comes from B; grlbwt_ctx_destroy releases the handles still alive.  grlbwt_merge_files: both
 * images from files, the merged image to a file (pinned reader and writer of the other file calls).
 * (GRLBWT_MERGE_ROUND=sort in the environment runs a round as gathered keys and a stable radix sort instead of the fused
 * kernels: the same merge, the form the kernels are measured against.) */
typedef struct grlbwt_merge grlbwt_merge;
typedef struct grlbwt_merge_info {
    uint64_t n_syms_a, n_syms_b, n_strings_a, n_strings_b;
    uint64_t sigma, separator;          /* distinct symbols of both images together; the common smallest one */
    uint64_t rounds;                    /* refinement rounds run, the one that changed nothing included */
    uint64_t rows_changed;              /* summed over the rounds: what a work-skipping form would have to touch */
    uint64_t n_runs, out_bytes, sb, fb; /* of the merged image */
    uint64_t idx_bytes, tile_rows;      /* 4 or 8; merged rows per workgroup tile of the round kernels */
    uint64_t scratch_bytes, held_bytes; /* peak scratch while merging; bytes the handle keeps */
} grlbwt_merge_info;
int grlbwt_merge_create(grlbwt_ctx *ctx, const void *dev_image_a, uint64_t bytes_a, const void *dev_image_b, uint64_t bytes_b,
                        int cell_bytes, uint64_t max_rounds /* 0: n + 2 */, grlbwt_merge **out);
int grlbwt_merge_info_get(const grlbwt_merge *mg, grlbwt_merge_info *out);
int grlbwt_merge_emit(grlbwt_ctx *ctx, const grlbwt_merge *mg, void *dev_out, uint64_t capacity_bytes);
int grlbwt_merge_interleave(grlbwt_ctx *ctx, const grlbwt_merge *mg, uint64_t *dev_bits);
int grlbwt_merge_destroy(grlbwt_ctx *ctx, grlbwt_merge *mg);
int grlbwt_merge_files(grlbwt_ctx *ctx, const char *path_a, const char *path_b, int cell_bytes, uint64_t max_rounds,
                       const char *path_out, grlbwt_merge_info *info /* may be NULL */);

/* ---- removing or keeping chosen strings: the image of a collection without the listed strings -- or of the listed strings
 * alone (GRLBWT_SELECT_KEEP) -- from its image, without the text.  With the merge this makes an image a collection that can be
 * maintained: add with merge, retire with select.  The suffixes of string i are the rows on the LF chain from row i (rows
 * [0, n_strings) are the terminators, in string order) to the row whose symbol is the separator; two remaining suffixes compare
 * as before, so deleting the chain rows of the listed strings leaves the BWT of the others, and the deleted rows, in order, are
 * the BWT of the listed strings.
 * INPUT: any well-formed image ("Accepted input" above), taken to be a BCR BWT as the inverters take it.  dev_ids: string numbers
 * in input order, as grlbwt_fm_locate reports them, in any order, repeats allowed -- the list is a set; n_ids = 0 is legal.  An
 * entry >= n_strings_in fails the whole call with GRLBWT_EINVAL; the message names the first such entry.
 * OUTPUT: the image of the remaining strings in their old relative order (the m-th remaining string in ascending old number
 * becomes string m).  When the input was built by this engine with cells of cell_bytes, the output is byte for byte what
 * grlbwt_build writes for the text of the remaining strings, header included: sb from the largest REMAINING symbol + 4, fb from
 * the largest total of one symbol (cell_bytes 1) or from the remaining length (2, 4, 8) -- the merge's rule.  The output always
 * has maximal runs and no empty record; removing nothing gives the canonical re-encoding of the input.
 * COST: one LF walk over the listed strings (always the LISTED ones: keeping 10 strings of a million costs 10 walks) and one pass
 * over the runs -- the per-string cost model of grlbwt_fm_locate.  GRLBWT_SELECT_CHECKPOINTS marks through the checkpointed
 * segments of grlbwt_invert_image_checkpointed instead (one checkpoint in 2^sample_bits rows, 0: the default): a segment walk
 * over the whole collection whatever the list holds, and the only form that ends for collections of long strings.  The marking
 * walk obeys GRLBWT_WALK_LANES.
 * GRLBWT_EINVAL: a result without any string (everything removed, or keeping an empty list), an image without a record or with
 * a bad header, cell_bytes not in {1, 2, 4, 8}, a symbol that does not fit cell_bytes, sample_bits without the checkpoint flag or
 * above 20, unknown flag bits, a marking walk that meets no separator (or checkpoint) in n steps (not the BWT of a collection),
 * capacity_bytes < out_bytes (nothing is written).  GRLBWT_ERANGE: 2^40 rows or more.  GRLBWT_ENOMEM: the structures do not fit
 * the free device memory (checked before the first walk; scratch_bytes).  64-bit positions from 2^32 - 256 rows on or with
 * GRLBWT_FLAG_FORCE_IDX64.  On every refusal *out = NULL and nothing is held.
 * grlbwt_select_create copies what it needs -- the image and the list may be freed when it returns -- and runs the walks and the
 * rewrite; the handle keeps the new runs, the values of a compacted alphabet and the marked rows (held_bytes).
 * grlbwt_select_emit writes the image (out_bytes of the info); grlbwt_select_rows the marked rows as ceil(n_syms_in / 64) words,
 * bit p of word p / 64 set when row p of the input BWT lies on a LISTED string's chain (the keep flag does not change the
 * bits); grlbwt_ctx_destroy releases the handles still alive.  grlbwt_select_files: the image from a file, the list from host
 * memory, the result to a file. */
typedef struct grlbwt_select grlbwt_select;
#define GRLBWT_SELECT_KEEP 1u              /* only the listed strings stay; without it the listed strings are removed */
#define GRLBWT_SELECT_CHECKPOINTS 2u       /* mark through checkpointed segments: collections of long strings */
#define GRLBWT_SELECT_SAMPLE_BITS(b) ((uint32_t)(b) << 8)   /* with CHECKPOINTS; 0 = the default, 1..20 */
typedef struct grlbwt_select_info {
    uint64_t n_syms_in, n_strings_in, n_runs_in;     /* rows, separators, non-empty records of the input */
    uint64_t n_listed;                               /* DISTINCT ids listed */
    uint64_t rows_marked, longest_walk;              /* rows on the listed strings' chains; LF steps of the longest marking walk (string or segment) */
    uint64_t n_syms_out, n_strings_out, n_runs_out, out_bytes, sb, fb;
    uint64_t separator, idx_bytes, flags;
    uint64_t walk_lanes, lane_refills;               /* of the marking walk, as in grlbwt_walk_info */
    uint64_t sample_bits, n_checkpoints, jump_rounds;/* 0 without CHECKPOINTS */
    uint64_t scratch_bytes, held_bytes;
} grlbwt_select_info;
int grlbwt_select_create(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes, const uint64_t *dev_ids,
                         uint64_t n_ids, uint32_t select_flags, grlbwt_select **out);
int grlbwt_select_info_get(const grlbwt_select *sel, grlbwt_select_info *out);
int grlbwt_select_emit(grlbwt_ctx *ctx, const grlbwt_select *sel, void *dev_out, uint64_t capacity_bytes);
int grlbwt_select_rows(grlbwt_ctx *ctx, const grlbwt_select *sel, uint64_t *dev_bits /* ceil(n_syms_in / 64) words */);
int grlbwt_select_destroy(grlbwt_ctx *ctx, grlbwt_select *sel);
int grlbwt_select_files(grlbwt_ctx *ctx, const char *path_in, const uint64_t *host_ids, uint64_t n_ids, int cell_bytes,
                        uint32_t select_flags, const char *path_out, grlbwt_select_info *info /* may be NULL */);

/* ---- inspection (parity tests; need GRLBWT_FLAG_KEEP_LEVELS) --------------- */
/* text of level >= 1 as (rank<<1 | rep) cells, the reference's on-disk parse format */
int grlbwt_level_text_size(const grlbwt_ctx *ctx, int level, uint64_t *n_cells);
int grlbwt_level_text_download(const grlbwt_ctx *ctx, int level, uint64_t *cells_out);
int grlbwt_level_bwt_size(const grlbwt_ctx *ctx, int level, uint64_t *n_runs);
int grlbwt_level_bwt_download(const grlbwt_ctx *ctx, int level, uint64_t *sym_out, uint64_t *len_out);

/* the level's grammar (produce_grammar, exact_par_phase.cpp:14-95: two cells per metasymbol, g1 >= sigma+3 = nested
 * metasymbol + sigma+3; has_hocc = phrases_has_hocc) and pre-BWT runs (produce_pre_bwt, :136-242: BWT marker = sigma+1,
 * hocc marker = sigma+2), i.e. the contents of the reference's dict_lev_r / pre_bwt_lev_r files.  Available for every
 * level once the parsing phase is done and until that level has been induced. */
int grlbwt_level_grammar_size(const grlbwt_ctx *ctx, int level, uint64_t *n_metasyms, uint64_t *prebwt_runs);
int grlbwt_level_grammar_download(const grlbwt_ctx *ctx, int level, uint64_t *g0, uint64_t *g1, uint8_t *has_hocc,
                                  uint64_t *prebwt_sym, uint64_t *prebwt_len);

int grlbwt_get_counters(const grlbwt_ctx *ctx, grlbwt_counters *out);
/* device memory taken by the engine's slab allocator: peak bytes in use, bytes reserved from the runtime */
int grlbwt_memory_usage(const grlbwt_ctx *ctx, uint64_t *peak_live_bytes, uint64_t *reserved_bytes);

/* ---- collection-level multi-GPU ------------------------
 * One context per GPU/process; the collection is sharded by record: rank g loads (text_upload /
 * text_attach_device) a contiguous range of whole strings, ranks in collection order.  The engine
 * calls back into the host for the exchanges (the host implements them with torch.distributed:
 * RCCL over xGMI on GPUs, gloo in the CPU tests); all pointers are device pointers of this
 * engine's device.  Replaces the thread-range strategy of mt_parse_strat_t
 * (include/parsing_strategies.h:200-275,277-386): hashing and parse emission stay local to the
 * shard, the per-thread table merge (join_thread_phrases) becomes an all-gather + device merge.
 * The output is the BWT of the WHOLE collection, identical on every rank and for every N.   */
typedef struct grlbwt_comm {
    int rank, size;
    void *user;
    /* every rank contributes `bytes` bytes at `send`; `recv` gets size*bytes in rank order; 0 = ok */
    int (*allgather)(void *user, const void *send, void *recv, uint64_t bytes);
    /* variable all-to-all (MPI_Alltoallv shape, byte units, host arrays of `size` entries): send_bytes[g] bytes at
     * send + send_off[g] go to rank g; recv_bytes[g] bytes from rank g land at recv + recv_off[g].  The engine keeps every
     * block at or below 256 MiB (larger exchanges arrive as several calls; GRLBWT_A2A_BLOCK overrides the limit). */
    int (*alltoallv)(void *user, const void *send, const uint64_t *send_bytes, const uint64_t *send_off,
                     void *recv, const uint64_t *recv_bytes, const uint64_t *recv_off);
    /* GRLBWT_COMM_STREAM_ORDERED: the callbacks enqueue the exchange on the context's stream
     * (grlbwt_ctx_set_stream) and return without waiting; the engine then neither drains its stream
     * before a callback nor expects the data to be complete when it returns -- later work on the same
     * stream is ordered behind it (RCCL through torch.distributed with that stream current).
     * 0: the callback may use any stream or the host; the engine synchronises before calling it and
     * the callback returns only when `recv` is complete (gloo, host staging).                        */
    uint32_t flags;
} grlbwt_comm;
#define GRLBWT_COMM_STREAM_ORDERED 1u
/* GRLBWT_COMM_KEEP_PARTS: the image is NOT gathered at the end of the build; every rank keeps the part whose runs it induced --
 * bytes [offset, offset + bytes) of the image (grlbwt_result_part; rank 0's part starts with the 16-byte header), the parts in
 * rank order make up the file.  grlbwt_result_size still reports the whole image, grlbwt_result_device_ptr /
 * grlbwt_result_download give the part, grlbwt_result_write_part puts it at its offset of the output file: N ranks write one
 * file, nothing of the image crosses the fabric.  (The reference's writer is one stream: exact_ind_phase.cpp:287-361 fills
 * bwt_lev_0 front to back; the counterpart of its N threads here is N writers.) */
#define GRLBWT_COMM_KEEP_PARTS 2u
/* grl_bwt_algo over the sharded collection: par_phase with a dictionary merge per round, ind_phase, image */
int grlbwt_dist_build(grlbwt_ctx *ctx, const grlbwt_comm *comm);

/* The two callbacks over RCCL inside the library, for hosts without a communication framework of their own (the grlbwt
 * executable's --gpus N: one process per GPU, the counterpart of `-t N` reaching mt_parse_strat_t in the reference,
 * main.cpp:62, parsing_strategies.h:200-275).  librccl is loaded on first use.  ONE rank makes the 128-byte id and the
 * host hands it to the others (shared memory, a pipe, a file); comm_create is collective over all `size` ranks, each
 * with its own device, and fills *comm with stream-ordered callbacks: ncclAllGather, and one grouped ncclSend/ncclRecv
 * per peer for the all-to-all, enqueued on the context's stream. */
#define GRLBWT_RCCL_ID_BYTES 128
int grlbwt_rccl_unique_id(void *id128);
int grlbwt_rccl_comm_create(grlbwt_ctx *ctx, const void *id128, int rank, int size, grlbwt_comm *comm);
int grlbwt_rccl_comm_destroy(grlbwt_comm *comm);

/* per-kernel timing with HIP events on the engine's stream (bench.py's roofline leg).
 * enable(1) clears the table and starts recording; dump writes one line per kernel name:
 * "<name> <launches> <total_ms> <algorithmic_bytes>\n" (NUL terminated, truncated to capacity; bytes = 0 where
 * the launch site states none; names carry "#<level>"). */
int grlbwt_profile_enable(grlbwt_ctx *ctx, int on);
int grlbwt_profile_dump(grlbwt_ctx *ctx, char *buf, uint64_t capacity);

/* device self-test of the primitives (scan, radix sort, ballot bit-vectors) against
 * host loops on seeded data; returns 0 or the index (<0) of the failing check */
int grlbwt_selftest(grlbwt_ctx *ctx, uint64_t n, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* GRLBWT_HIP_H */
