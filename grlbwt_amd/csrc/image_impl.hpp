// image_impl.hpp -- the consumers of a finished .rl_bwt image: what reads, inverts, searches, merges or rewrites
// an image in device memory.  Nothing here builds a BWT and the builder (engine_impl.hpp) calls nothing of it.
//
// Included once per index width right after engine_impl.hpp, inside the same GRL_NS / GRL_IDX_T window: engine_hip.hip and
// tests/hostsim/engine_sim.cpp do so.  engine_impl.hpp also ends with this include, so that a translation unit that names
// engine_impl.hpp alone still gets what capi_impl.hpp calls; the guard below makes the second inclusion of a width empty.
//
// What it holds: the device functors (in the order of the sections below) and, as static members of the stateless
// `struct Image`, the host functions behind the C-ABI's grlbwt_image_*, grlbwt_invert_*, grlbwt_fm_*, grlbwt_docs_*, grlbwt_merge_*
// and grlbwt_select_* calls (reference: scripts/*.cpp of ddiazdom/grlBWT):
//   records and the scripts/ consumers   ImageRecs, plain / rle / stats / split_runs
//   inversion                            per position (invert_t) and per run (RunIndex, invert_runs_t)
//   FM index                             count, locate, match / MEMs, extract, the LCP array (FmLcp), the k-mer table (fm_kmers)
//   the strings behind row ranges        ImageDocs: the document array kept with PREV (and LST, START), docs_create / docs_query
//   checkpointed LF walks                lf_checkpoints and the walks cut at checkpoints
//   merge, select                        ImageMerge, ImageSelect
// The pieces every consumer shares, one copy each: ImageRecs (the record layout), image_header / check_cell_bytes /
// with_cell (opening an image), drop_empty_runs, run_index_load / run_index_lf, LfRows (one LF step), SymOut (rank -> cell).
//
// What it takes from engine_impl.hpp, all at namespace level: DBuf, RankBits / build_rankbits / rank1 / RankCell, Runs /
// merge_runs, alphabet_compact, the record writers PackRunsFn / RunRecordFn / RunLen, the input functors IdxIn / IdxIn64 /
// CellIn / PopcIn / PtrU32In / SymHeadIn64, upper_bound / lower_bound and bitlen64.

#if (GRL_IDX_BYTES == 4 && !defined(GRL_IMAGE_IMPL_32)) || (GRL_IDX_BYTES == 8 && !defined(GRL_IMAGE_IMPL_64))
#if GRL_IDX_BYTES == 4
#define GRL_IMAGE_IMPL_32
#else
#define GRL_IMAGE_IMPL_64
#endif

namespace GRL_NS {

// ---- .rl_bwt consumers (scripts/grl2plain.cpp, scripts/reverse_bwt.cpp + fm_index.h:79-83) ------
struct SepLenIn {         // total length of the runs of one symbol
    const u32 *sym; const idx_t *len; u32 code;
    GRL_DEV u64 operator()(u64 i) const { return sym[i] == code ? (u64)len[i] : 0ull; }
};
// The packed records of an image, behind its 16 header bytes: (symbol: sb bytes, length: fb bytes), both little-endian.  The
// one place that knows the layout on the reading side (PackRunsFn and RunRecordFn of engine_impl.hpp write it).
struct ImageRecs {
    const u8 *img; u32 sb, fb;
    GRL_DEV static u64 le(const u8 *p, u32 w) {
        u64 v = 0;
        for (u32 b = 0; b < w; b++) v |= (u64)p[b] << (8 * b);
        return v;
    }
    GRL_DEV const u8 *at(u64 i) const { return img + 16 + i * (u64)(sb + fb); }
    GRL_DEV u64 sym(u64 i) const { return le(at(i), sb); }       // all 64 bits of it
    GRL_DEV u64 len(u64 i) const { return le(at(i) + sb, fb); }
};
template <class sym_t>
struct UnpackRunsFn {     // records -> arrays (sym_t = u32: the symbol's low half; u64: all of it)
    ImageRecs in; sym_t *sym; idx_t *len;
    GRL_DEV void operator()(u64 i) const { sym[i] = (sym_t)in.sym(i); len[i] = (idx_t)in.len(i); }
};
struct NonEmptyIn {        // 1 for a record that holds symbols
    const idx_t *len;
    GRL_DEV idx_t operator()(u64 i) const { return len[i] != 0 ? (idx_t)1 : (idx_t)0; }
};
template <class sym_t>
struct KeepRunsFn {        // compacting copy of the non-empty records (dst = scan of NonEmptyIn)
    const sym_t *sym; const idx_t *len; const idx_t *dst; sym_t *osym; idx_t *olen;
    GRL_DEV void operator()(u64 i) const {
        const idx_t l = len[i];
        if (l != 0) { const u64 o = dst[i]; osym[o] = sym[i]; olen[o] = l; }
    }
};
struct ImageSymIn {        // run symbol straight from the packed records
    ImageRecs in;
    GRL_DEV u64 operator()(u64 i) const { return in.sym(i); }
};
struct UnpackSymFn {
    ImageRecs in; u64 *sym;
    GRL_DEV void operator()(u64 i) const { sym[i] = in.sym(i); }
};
struct ImageLenIn {        // run length straight from the packed records (64-bit sum: decides the index width of a consumer)
    ImageRecs in;
    GRL_DEV u64 operator()(u64 i) const { return in.len(i); }
};
// scripts/grl2plain.cpp:30-45: one output byte per BWT position, (char)sym, optional null replacement.  The replacement is
// decided per RUN on all 64 bits of the symbol (a symbol of 2^32 is not the null character; its low byte is 0 all the same).
struct PlainSymFn {
    ImageRecs in; int null_char; u32 *rsym;
    GRL_DEV void operator()(u64 i) const {
        const u64 s = in.sym(i);
        rsym[i] = (s == 0 && null_char >= 0) ? (u32)null_char : (u32)(u8)s;
    }
};
struct PlainRunsFn {
    const u32 *rsym; const u64 *rw; const idx_t *rb; u8 *out;
    GRL_DEV void operator()(u64 i) const { out[i] = (u8)rsym[rank1(rw, rb, i + 1) - 1]; }
};
struct RleExportFn {      // scripts/grlbwt2rle.cpp:22-30: .syms as uint8, .len as uint32 (the reference's casts)
    const u32 *rsym; const idx_t *rlen; u8 *syms; u32 *lens;
    GRL_DEV void operator()(u64 i) const { syms[i] = (u8)rsym[i]; lens[i] = (u32)rlen[i]; }
};
// split_runs (scripts/split_runs.cpp:44-109).  A run is first cut into pieces of at most L = 2^bits - 1 symbols
// (`while(len>max_length)`), every piece then at the multiples of the block size B that fall strictly inside it; a piece
// that STARTS on a block boundary (other than position 0) is preceded by a zero-length record of its own symbol (the
// reference arrives there with acc_block == block_size and emits `push_back(sym, 0)`, :87-90).  Each boundary in (0, n)
// therefore costs exactly one extra record, so the first record of piece j of run i sits at
//   (#pieces before it) + (#multiples of B in (0, start of the piece)).
// An EMPTY input record is one piece and one output record wherever it lies: on a boundary it pays nothing (the next
// non-empty piece starts there too and pays), so it must not write the extra record -- that slot belongs to its successor,
// or lies behind the output when nothing follows.
struct PieceCountFn {     // number of L-pieces of every run
    const idx_t *len; u64 L;
    GRL_DEV idx_t operator()(u64 i) const { u64 l = len[i]; return (idx_t)(l == 0 ? 1 : (l + L - 1) / L); }
};
struct SplitRunsFn {      // one lane per L-piece
    const u32 *rsym; const idx_t *rlen; const idx_t *rpos; const idx_t *jbase; const u64 *jw; const idx_t *jb;
    u64 L, B;
    u32 *osym; idx_t *olen;
    GRL_DEV void operator()(u64 x) const {
        const u64 i = rank1(jw, jb, x + 1) - 1;          // run owning piece x
        const u64 j = x - (u64)jbase[i];
        const u64 l = rlen[i];
        const u64 k = l == 0 ? 0 : (l + L - 1) / L - 1;  // full pieces peeled off in front of the remainder
        u64 cur = (u64)rpos[i] + j * L;
        const u64 end = cur + (j < k ? L : l - k * L);
        const u32 sy = rsym[i];
        u64 o = x + ((B && cur > 0) ? (cur - 1) / B : 0);
        if (B) {
            if (cur > 0 && cur % B == 0 && end > cur) { osym[o] = sy; olen[o] = 0; o++; }     // (an empty record is its own zero-length record)
            for (u64 nb = (cur / B + 1) * B; nb < end; nb += B) { osym[o] = sy; olen[o] = (idx_t)(nb - cur); o++; cur = nb; }
        }
        osym[o] = sy; olen[o] = (idx_t)(end - cur);
    }
};
struct RunSymFn {         // for_each_agg protocol: every run is a work item, its bucket is its symbol
    static constexpr int kBatch = 1;
    static constexpr bool kClaims = false;
    GRL_DEV u64 claim_pos(u64 i) const { return i; }
    const u32 *rsym;
    GRL_DEV bool is_start(u64) const { return true; }
    GRL_DEV u32 process(u64 i) const { return rsym[i]; }
    GRL_DEV u32 operator()(u64 i) const { return rsym[i]; }
};
struct BinAddFn {
    u64 *bins;
    GRL_DEV void operator()(u32 b, u32 c) const { prim::atomic_add(&bins[b & 255u], (u64)c); }
};
struct LenFitIn {         // 1 if the run length needs exactly `cls` bytes class (1: <=255, 2: <=65535, 3: more)
    const idx_t *len; int cls;
    GRL_DEV u64 operator()(u64 i) const {
        u64 l = len[i];
        int c = l <= 255 ? 1 : (l <= 65535 ? 2 : 3);
        return c == cls ? 1ull : 0ull;
    }
};
struct LenKeyFn {
    const idx_t *len; u32 *key; u32 *val;
    GRL_DEV void operator()(u64 i) const { key[i] = (u32)len[i]; val[i] = (u32)i; }
};
struct ExpandRunsFn {     // grl2plain: symbol of every BWT position through the run-start bitmap
    const u32 *rsym; const u64 *rw; const idx_t *rb; u32 *out; idx_t *idx;
    GRL_DEV void operator()(u64 i) const { out[i] = rsym[rank1(rw, rb, i + 1) - 1]; idx[i] = (idx_t)i; }
};
struct LfScatterFn {      // LF[order[j]] = j  (order = stable sort of positions by symbol)
    const idx_t *order; idx_t *lf;
    GRL_DEV void operator()(u64 j) const { lf[order[j]] = (idx_t)j; }
};
struct InvertLenFn {      // string i: backward LF walk from row i until its own terminator comes back
    const u32 *bwt; const idx_t *lf; u32 sep; idx_t *slen;
    GRL_DEV void operator()(u64 i) const {
        u64 row = i, l = 1;
        for (u32 c = bwt[row]; c != sep; c = bwt[row]) { l++; row = lf[row]; }
        slen[i] = (idx_t)l;
    }
};
template <class cell_t>
struct SymOut {             // the cell a walk writes for symbol c (alpha: the values of a compacted alphabet, the walk runs on their ranks; null: the symbols themselves)
    const u64 *alpha;
    GRL_DEV cell_t operator()(u32 c) const { return alpha ? (cell_t)alpha[c] : (cell_t)c; }
};
template <class cell_t>
struct InvertWriteFn {
    const u32 *bwt; const idx_t *lf; const idx_t *off; u32 sep; cell_t *text; SymOut<cell_t> val;
    GRL_DEV void operator()(u64 i) const {
        u64 end = off[i + 1] - 1, row = i;
        text[end] = val(sep);
        for (u32 c = bwt[row]; c != sep; c = bwt[row]) { text[--end] = val(c); row = lf[row]; }
    }
};

// ---- the same inversion indexed by RUNS (scripts/fm_index.h:79-83 computes LF from the symbol's rank; over the run-length
// BWT the rank of a run's first symbol is a prefix sum over the RUNS of that symbol).  A stable sort of the runs by symbol and
// a scan of their lengths in that order give LF of every run start; LF inside a run is linear, so one record per run --
// (LF(start) - start, symbol) -- and the run-start bit-vector replace the per-position arrays: 28-36 bytes per RUN instead
// of 20-36 per symbol, which is what lets the 10 GB headline image (1.66 G runs, 10^10 symbols) round-trip on one device.
template <int IB> struct RunRecT;
template <> struct alignas(8) RunRecT<4> { u32 delta; u32 sym; };
template <> struct alignas(16) RunRecT<8> { u64 delta; u32 sym; u32 pad; };
typedef RunRecT<sizeof(idx_t)> RunRec;
struct RankCellFn {
    const u64 *words; const idx_t *base; RankCell *rc;
    GRL_DEV void operator()(u64 i) const { rc[i] = RankCell{words[i], (u64)base[i]}; }
};
struct IotaFn {
    idx_t *v;
    GRL_DEV void operator()(u64 i) const { v[i] = (idx_t)i; }
};
struct RunOrderLenIn {    // length of the j-th run in (symbol, position) order
    const idx_t *rlen; const idx_t *order;
    GRL_DEV idx_t operator()(u64 j) const { return rlen[order[j]]; }
};
struct RunLfEmitFn {      // emit side of that scan: ex = LF of the run's first position
    static constexpr bool kWaveEmit = false;
    const idx_t *order; const idx_t *rpos; const u32 *rsym; RunRec *rec;
    GRL_DEV void operator()(u64 j, idx_t ex, idx_t) const {
        const u64 k = order[j];
        RunRec r;
        r.delta = (decltype(r.delta))(ex - rpos[k]);      // (wraps below zero: row + delta is taken modulo 2^bits)
        r.sym = rsym[k];
        rec[k] = r;
    }
};
GRL_DEV u64 run_of_row(const RankCell *rc, u64 row) {      // index of the run holding BWT position row
    const RankCell c = rc[(row + 1) >> 6];
    return c.b + (u64)__builtin_popcountll(c.w & ((1ull << ((row + 1) & 63)) - 1ull)) - 1;
}
// LF of any row, for the row's OWN symbol: the run-start bit-vector with the rank of every word, and one record per run.
struct LfRows {
    const RankCell *rc; const RunRec *rec;
    GRL_DEV RunRec at(idx_t row) const { return rec[run_of_row(rc, (u64)row)]; }
    GRL_DEV static idx_t next(idx_t row, const RunRec &r) { return (idx_t)(row + (idx_t)r.delta); }      // (modulo 2^bits: RunLfEmitFn)
};
struct RunInvertLenFn {
    LfRows lf; u32 sep; idx_t *slen;
    GRL_DEV void operator()(u64 i) const {
        idx_t row = (idx_t)i;
        u64 l = 1;
        RunRec r = lf.at(row);
        while (r.sym != sep) { l++; row = LfRows::next(row, r); r = lf.at(row); }
        slen[i] = (idx_t)l;
    }
};
template <class cell_t>
struct RunInvertWriteFn {
    LfRows lf; const idx_t *off; u32 sep; cell_t *text; SymOut<cell_t> val;
    GRL_DEV void operator()(u64 i) const {
        u64 end = off[i + 1] - 1;
        idx_t row = (idx_t)i;
        text[end] = val(sep);
        RunRec r = lf.at(row);
        while (r.sym != sep) { text[--end] = val(r.sym); row = LfRows::next(row, r); r = lf.at(row); }
    }
};

template <class cell_t>
struct RunInvertTailFn {    // the last `tail` cells of string i (separator included), right-aligned in slot i of `tail` cells; the rest of the slot stays as it was
    LfRows lf; u32 sep; u64 tail; cell_t *out; idx_t *got; SymOut<cell_t> val;
    GRL_DEV void operator()(u64 i) const {
        u64 end = (i + 1) * tail - 1, l = 1;
        idx_t row = (idx_t)i;
        out[end] = val(sep);
        RunRec r = lf.at(row);
        while (r.sym != sep && l < tail) { out[--end] = val(r.sym); l++; row = LfRows::next(row, r); r = lf.at(row); }
        got[i] = (idx_t)l;
    }
};

// ---- merging two images (grlbwt_merge_*): the interleave z holds one flag byte per merged row, 0 = the row is the
// next unread row of A, 1 = of B; ra / rb hold one rank byte per row of A / B (the rank of the row's symbol among the distinct
// values of both images).
struct MgExpandFn {        // one rank byte per row, through the run-start bitmap
    const u32 *rrank; const u64 *rw; const idx_t *rb; u8 *out;
    GRL_DEV void operator()(u64 i) const { out[i] = (u8)rrank[rank1(rw, rb, i + 1) - 1]; }
};
struct MgSplitFn {         // z[p] = p >= na: 0^na 1^(n - na) -- the first interleave, and the separator bucket of every round
    u8 *z; u64 na;
    GRL_DEV void operator()(u64 p) const { z[p] = p >= na ? (u8)1 : (u8)0; }
};
struct MgFlagPred {
    const u8 *z;
    GRL_DEV bool operator()(u64 p) const { return z[p] != 0; }
};
struct MgDiffIn {
    const u8 *a, *b;
    GRL_DEV u64 operator()(u64 p) const { return a[p] != b[p] ? 1ull : 0ull; }
};
struct MgSym {             // the merged symbol (a rank) of row p through the interleave as a bit-vector with ranks
    const u8 *ra, *rb; const u64 *zw; const idx_t *zb;
    GRL_DEV u32 operator()(u64 p) const {
        const u64 b = rank1(zw, zb, p);                  // B-rows in front of p
        return ((zw[p >> 6] >> (p & 63)) & 1ull) ? (u32)rb[b] : (u32)ra[p - b];
    }
};
struct MgKeyFn {           // the serial form of a round: the merged symbols gathered as sort keys
    MgSym s; u8 *key;
    GRL_DEV void operator()(u64 p) const { key[p] = (u8)s(p); }
};
struct MgHeadPred {
    MgSym s;
    GRL_DEV bool operator()(u64 p) const { return p == 0 || s(p) != s(p - 1); }
};
struct MgHeadFn {          // for_each_set_bit over the run heads: run `ord` starts at row p
    MgSym s; u32 *sym; idx_t *start;
    GRL_DEV void operator()(u64 p, u64 ord) const { sym[ord] = s(p); start[ord] = (idx_t)p; }
};

// ---- counting and locating patterns: one step past scripts/fm_index.h, which stops at lf().  RunRec answers LF for a row's OWN
// symbol; a backward search needs rank_c(p), the number of c in BWT[0, p), for any c.  The runs in (symbol, position) order --
// the order the sort above makes -- answer it by binary search: key[j] = (symbol, start) of the j-th run in that order,
// slf[j] = symbols in the runs before it (slf[R] = n), so slf at the first run of c is C[c], the symbols smaller than c.
template <int IB> struct FmKeyT;
template <> struct FmKeyT<4> {                 // symbol << 32 | start: one word while positions have 32 bits
    u64 v;
    GRL_DEV static FmKeyT make(u32 sym, u64 start) { return FmKeyT{(u64)sym << 32 | start}; }
    GRL_DEV u32 sym() const { return (u32)(v >> 32); }
    u32 host_sym() const { return (u32)(v >> 32); }           // (of a key copied to the host)
    GRL_DEV u64 start() const { return v & 0xFFFFFFFFull; }
    GRL_DEV bool below(u32 c, u64 p) const { return v < ((u64)c << 32 | p); }       // sorts in front of (c, p)
};
template <> struct alignas(16) FmKeyT<8> {
    u64 st, sy;
    GRL_DEV static FmKeyT make(u32 sym, u64 start) { return FmKeyT{start, (u64)sym}; }
    GRL_DEV u32 sym() const { return (u32)sy; }
    u32 host_sym() const { return (u32)sy; }
    GRL_DEV u64 start() const { return st; }
    GRL_DEV bool below(u32 c, u64 p) const { return sy < (u64)c || (sy == (u64)c && st < p); }
};
typedef FmKeyT<sizeof(idx_t)> FmKey;
struct FmKeyEmitFn {      // RunLfEmitFn that also keeps the sorted order itself (rec may be null: no walk wanted)
    static constexpr bool kWaveEmit = false;
    const idx_t *order; const idx_t *rpos; const u32 *rsym; RunRec *rec; FmKey *key; idx_t *slf;
    GRL_DEV void operator()(u64 j, idx_t ex, idx_t) const {
        const u64 k = order[j];
        key[j] = FmKey::make(rsym[k], (u64)rpos[k]);
        slf[j] = ex;
        if (rec) {
            RunRec r;
            r.delta = (decltype(r.delta))(ex - rpos[k]);
            r.sym = rsym[k];
            rec[k] = r;
        }
    }
};
struct FmHeadIn {         // 1 where a sorted run has another symbol than the run in front of it: their number is sigma
    const FmKey *key;
    GRL_DEV u64 operator()(u64 j) const { return j == 0 || key[j].sym() != key[j - 1].sym() ? 1ull : 0ull; }
};
struct FmNoTop {          // the search without a top level (the LDS one: prim::LdsTop)
    GRL_DEV void narrow(u32, u64, u64 &, u64 &) const {}
};
// ONE step of the backward search for symbol c: both ends of [lo, hi) go from a row p to C[c] + rank_c(p).  j = the keys below
// (c, p); the run in front of it, when it is a run of c, is the last run of c that starts before p and holds min(p - start, length)
// of the symbols counted; otherwise no run of c starts before p and the answer is slf[j] = C[c].  Each lower bound halves
// [a, b] at most 64 times; hi's starts at lo's (hi >= lo).
template <class TOP>
GRL_DEV void fm_step(const FmKey *key, const idx_t *slf, u64 R, const TOP &top, u32 c, u64 &lo, u64 &hi) {
    u64 from = 0;
    auto end = [&](u64 p) {
        u64 a = from, b = R;
        top.narrow(c, p, a, b);
        for (int it = 0; it < 64 && a < b; it++) { const u64 mid = (a + b) >> 1; if (key[mid].below(c, p)) a = mid + 1; else b = mid; }
        const u64 j = from = a;
        u64 r = (u64)slf[j];
        if (j > 0) {
            const FmKey q = key[j - 1];
            if (q.sym() == c) { const u64 base = (u64)slf[j - 1], len = r - base, in = p - q.start(); r = base + (in < len ? in : len); }
        }
        return r;
    };
    lo = end(lo);
    hi = end(hi);
}
// pattern i = cells [off[i], off[i + 1]) of w bytes each, read as values; their symbols are the values themselves or, for an
// image with a compacted alphabet, the ranks among alpha[0, sigma).  A value that is no symbol empties the range.
struct FmCountFn {
    typedef FmKey Key;
    const FmKey *key; const idx_t *slf; u64 R, n;
    const u64 *alpha; u64 sigma;
    const void *cells; int w; const u64 *off; u64 *lo, *hi;
    GRL_HD const FmKey *keys() const { return key; }
    GRL_HD u64 n_keys() const { return R; }
    GRL_DEV u64 cell(u64 x) const {
        switch (w) {
            case 1: return (u64)((const u8 *)cells)[x];
            case 2: return (u64)((const u16 *)cells)[x];
            case 4: return (u64)((const u32 *)cells)[x];
            default: return ((const u64 *)cells)[x];
        }
    }
    GRL_DEV bool code(u64 v, u32 &c) const {
        if (!alpha) { c = (u32)v; return (v >> 32) == 0; }
        u64 a = 0, b = sigma;
        for (int it = 0; it < 64 && a < b; it++) { const u64 mid = (a + b) >> 1; if (alpha[mid] < v) a = mid + 1; else b = mid; }
        c = (u32)a;
        return a < sigma && alpha[a] == v;
    }
    template <class TOP>
    GRL_DEV void operator()(u64 i, const TOP &top) const {
        u64 a = 0, b = n;
        const u64 x0 = off[i];
        for (u64 x = off[i + 1]; x > x0 && a < b; x--) {       // (at most the pattern's cells)
            u32 c;
            if (!code(cell(x - 1), c)) { b = a; break; }
            fm_step(key, slf, R, top, c, a, b);
        }
        if (a >= b) a = b = 0;
        lo[i] = a; hi[i] = b;
    }
};
struct FmCountPlainFn {   // the same through prim::for_each, without a top level
    FmCountFn f;
    GRL_DEV void operator()(u64 i) const { f(i, FmNoTop{}); }
};
struct FmOffsetsBadIn {
    const u64 *off;
    GRL_DEV u64 operator()(u64 i) const { return off[i] > off[i + 1] ? 1ull : 0ull; }
};
struct FmSepMisuseIn {    // cell x0 + k: the number of its pattern when it holds the separator and is not the pattern's last cell, else ~0
    FmCountFn f; u64 sepval, x0, np;
    GRL_DEV u64 operator()(u64 k) const {
        const u64 x = x0 + k;
        if (f.cell(x) != sepval) return ~0ull;
        const u64 i = upper_bound<u64>(f.off, np + 1, x) - 1;      // off[i] <= x < off[i + 1]: empty patterns are stepped over
        return x + 1 == f.off[i + 1] ? ~0ull : i;
    }
};
// ---- longest matches and maximal exact matches (grlbwt_fm_match / grlbwt_fm_mems).  Ticket t is the query cell
// x = x0 + t, at offset e inside its pattern: the greedy backward search from [0, n) over cells x, x - 1, ... keeps the last
// non-empty range, so len is the largest L <= min(e + 1, max_len) such that the L cells ending at x occur in the collection
// (occurring is monotone in L).  A cell that is no symbol, or the separator, ends the item: no match holds or crosses one.
//   Loops: an item takes at most min(e + 1, max_len) steps, each one fm_step; begin's upper_bound halves n_patterns + 1 offsets.
struct FmMatchFn {
    typedef FmKey Key;
    struct State { u64 x, lo, hi, len, cap; };
    FmCountFn f; u64 sepval, x0, np, max_len; u64 *len, *lo, *hi;       // (lo and hi both null: the lengths alone)
    GRL_HD const FmKey *keys() const { return f.key; }
    GRL_HD u64 n_keys() const { return f.R; }
    GRL_DEV bool begin(u64 t, State &st) const {
        st.x = x0 + t;
        const u64 i = upper_bound<u64>(f.off, np + 1, st.x) - 1;      // off[i] <= x < off[i + 1]: empty patterns are stepped over
        st.cap = st.x - f.off[i] + 1;
        if (max_len && max_len < st.cap) st.cap = max_len;
        st.lo = 0; st.hi = f.n; st.len = 0;
        return true;
    }
    template <class TOP>
    GRL_DEV bool step(State &st, const TOP &top) const {
        const u64 v = f.cell(st.x - st.len);
        u32 c;
        if (st.lo >= st.hi || v == sepval || !f.code(v, c)) return true;       // (an index of no symbol: nothing matches)
        u64 a = st.lo, b = st.hi;
        fm_step(f.key, f.slf, f.R, top, c, a, b);
        if (a >= b) return true;
        st.lo = a; st.hi = b; st.len++;
        return st.len >= st.cap;
    }
    GRL_DEV bool step(State &st) const { return step(st, FmNoTop{}); }
    GRL_DEV void end(u64 t, const State &st) const {
        len[t] = st.len;
        if (lo) { lo[t] = st.len ? st.lo : 0; hi[t] = st.len ? st.hi : 0; }
    }
};
struct FmMatchLaneFn {    // the same, one lane per cell through prim::top_search (GRLBWT_FM_MATCH=l)
    typedef FmKey Key;
    FmMatchFn f;
    GRL_HD const FmKey *keys() const { return f.keys(); }
    GRL_HD u64 n_keys() const { return f.n_keys(); }
    template <class TOP>
    GRL_DEV void operator()(u64 t, const TOP &top) const {
        FmMatchFn::State st;
        f.begin(t, st);
        while (!f.step(st, top)) {}
        f.end(t, st);
    }
};
struct FmLenCappedIn {
    const u64 *len; u64 cap;
    GRL_DEV u64 operator()(u64 t) const { return len[t] == cap ? 1ull : 0ull; }
};
// end e of a pattern closes a maximal match when its length is at least the floor and the next end's match is no longer:
// L[e + 1] <= L[e] + 1 always (drop the last cell of that match), with equality exactly when this one extends to the right
struct FmMemFlagIn {
    const u64 *len, *off; u64 x0, np, floor;
    GRL_DEV bool operator()(u64 t) const {
        const u64 L = len[t];
        if (L < floor) return false;
        const u64 x = x0 + t, i = upper_bound<u64>(off, np + 1, x) - 1;
        return x + 1 == off[i + 1] || len[t + 1] <= L;
    }
};
struct FmMemEmitFn {      // prim::for_each_set_bit over those flags: entry `ord` is the match that ends at cell x0 + t
    const u64 *len, *slo, *shi, *off; u64 x0, np; u64 *pat, *beg, *mlen, *lo, *hi;
    GRL_DEV void operator()(u64 t, u64 ord) const {
        const u64 x = x0 + t, i = upper_bound<u64>(off, np + 1, x) - 1, L = len[t];
        pat[ord] = i; beg[ord] = x - off[i] + 1 - L; mlen[ord] = L;
        if (lo) { lo[ord] = slo[t]; hi[ord] = shi[t]; }
    }
};
// ---- patterns with up to k substituted cells (grlbwt_fm_approx).  Ticket i is pattern i, of m cells.  The search
// runs from the pattern's last cell to its first; at a cell, with range r and d substitutions made, it first tries, while d < k,
// every symbol of the image above the separator other than the pattern's own cell in ascending order -- each one that leaves a
// non-empty range is followed with d + 1 -- and then the pattern's own cell with d.  The own cell comes last, so nothing has to
// be kept for it: the whole state is the current (x, lo, hi) and one Frame per substitution made, at most k = 3 of them, held in
// NAMED members among whose VALUES the depth chooses (an array indexed by it goes to scratch).  A cell that is no symbol, or
// the separator, has no own step: only a substitution passes it.  x = 0 is a hit: entry (d, [lo, hi), the frames' offsets and
// symbols).  The symbols present come from the keys: the next one above c is the symbol of the key at the lower bound of
// (c + 1, 0), one more search under the top level; no table is kept.
//   Two passes of this one search: cnt[i] = hits | cut << 63 while `mism` is null; then, with hoff = the scanned counts, the
//   entries, cnt[i] = the pass's backward steps, and `bad` where a pattern found another number of hits than it had counted.
//   The emit pass never stores past hoff[i + 1].  With max_hits the search ends at the first hit beyond it: that is what says
//   the list was longer.
//   Loops: step() holds none but the binary searches; over an item, steps per frame <= sigma, frames <= k, cells <= m.
struct FmApproxFn {
    typedef FmKey Key;
    struct Frame { u64 x, lo, hi; u32 cur; };      // the node where a substitution was made (x cells were left), and the substitute
    struct State {
        u64 x0, x, lo, hi, cnt, base, room, steps;
        u32 d, cur;                // substitutions made; the last substitute tried at this node (the separator: none yet)
        bool sub, cut;             // substitutes are still to be tried here; the list was cut at max_hits
        u64 x_0, x_1, x_2, lo_0, lo_1, lo_2, hi_0, hi_1, hi_2;      // the frames, member by member: every access names its member,
        u32 c_0, c_1, c_2;                                          // so that the state stays in registers
    };
    FmCountFn f; u32 sep; u64 sepval; u32 k; u64 max_hits;
    u64 *cnt; const u64 *hoff; u64 *mism, *lo, *hi, *spos, *sval; u32 *bad;
    GRL_HD const FmKey *keys() const { return f.key; }
    GRL_HD u64 n_keys() const { return f.R; }
    // Every member is read and written where it stands and the depth only chooses among VALUES: a store under a switch on the
    // depth is merged by the compiler into one store through a chosen address, and the frames are back in scratch.
    template <class T>
    GRL_DEV static T pick(u32 d, T a0, T a1, T a2) { return d == 0 ? a0 : d == 1 ? a1 : a2; }
    template <class T>
    GRL_DEV static void put(u32 d, T v, T &a0, T &a1, T &a2) {
        const T b0 = a0, b1 = a1, b2 = a2;
        a0 = d == 0 ? v : b0; a1 = d == 1 ? v : b1; a2 = d >= 2 ? v : b2;
    }
    GRL_DEV static void save(State &st, u32 d, const Frame &fr) {
        put(d, fr.x, st.x_0, st.x_1, st.x_2); put(d, fr.lo, st.lo_0, st.lo_1, st.lo_2);
        put(d, fr.hi, st.hi_0, st.hi_1, st.hi_2); put(d, fr.cur, st.c_0, st.c_1, st.c_2);
    }
    GRL_DEV static Frame load(const State &st, u32 d) {
        return Frame{pick(d, st.x_0, st.x_1, st.x_2), pick(d, st.lo_0, st.lo_1, st.lo_2), pick(d, st.hi_0, st.hi_1, st.hi_2),
                     pick(d, st.c_0, st.c_1, st.c_2)};
    }
    template <class TOP>
    GRL_DEV bool next_sym(u32 c, const TOP &top, u32 &out) const {      // the smallest symbol of the image above c
        if (c == ~0u) return false;
        u64 a = 0, b = f.R;
        top.narrow(c + 1, 0, a, b);
        for (int it = 0; it < 64 && a < b; it++) { const u64 mid = (a + b) >> 1; if (f.key[mid].below(c + 1, 0)) a = mid + 1; else b = mid; }
        if (a >= f.R) return false;
        out = f.key[a].sym();
        return true;
    }
    GRL_DEV void hit(State &st) const {
        if (max_hits && st.cnt == max_hits) { st.cut = true; return; }
        if (mism && st.cnt < st.room) {
            const u64 j = st.base + st.cnt;
            mism[j] = (u64)st.d; lo[j] = st.lo; hi[j] = st.hi;
            if (spos) {
#pragma unroll
                for (u32 s = 0; s < 3; s++) {                            // (k <= 3; unrolled: every load names its frame)
                    if (s >= k) break;
                    const Frame fr = load(st, s);
                    spos[j * k + s] = s < st.d ? fr.x - 1 : ~0ull;
                    sval[j * k + s] = s < st.d ? (f.alpha ? f.alpha[fr.cur] : (u64)fr.cur) : ~0ull;
                }
            }
        }
        st.cnt++;
    }
    // back to the node of the last substitution; true: there is none, the search is over
    GRL_DEV bool pop(State &st) const {
        if (st.d == 0) return true;
        st.d--;
        const Frame fr = load(st, st.d);
        st.x = fr.x; st.lo = fr.lo; st.hi = fr.hi; st.cur = fr.cur; st.sub = true;
        return false;
    }
    GRL_DEV bool enter(State &st) const {                                // a node was reached with a non-empty range
        if (st.x == 0) { hit(st); return st.cut || pop(st); }
        st.sub = st.d < k; st.cur = sep;
        return false;
    }
    GRL_DEV bool begin(u64 i, State &st) const {
        st.x0 = f.off[i]; st.x = f.off[i + 1] - st.x0;
        st.lo = 0; st.hi = f.n; st.cnt = 0; st.steps = 0; st.d = 0; st.cur = sep; st.sub = false; st.cut = false;
        st.base = mism ? hoff[i] : 0; st.room = mism ? hoff[i + 1] - st.base : 0;
        st.x_0 = st.x_1 = st.x_2 = st.lo_0 = st.lo_1 = st.lo_2 = st.hi_0 = st.hi_1 = st.hi_2 = 0; st.c_0 = st.c_1 = st.c_2 = 0;
        if ((st.x && st.lo >= st.hi) || enter(st)) { end(i, st); return false; }      // (an index of no symbol; a pattern of no cell)
        return true;
    }
    template <class TOP>
    GRL_DEV bool step(State &st, const TOP &top) const {                // at most ONE fm_step
        const u64 v = f.cell(st.x0 + st.x - 1);
        u32 qc = 0, c = 0;
        const bool own = f.code(v, qc) && v != sepval;
        bool have = false;
        if (st.sub) {
            have = next_sym(st.cur, top, c);
            if (have && own && c == qc) have = next_sym(qc, top, c);
            st.sub = have;
        }
        if (!have) {
            if (!own) return pop(st);
            c = qc;
        }
        u64 a = st.lo, b = st.hi;
        fm_step(f.key, f.slf, f.R, top, c, a, b);
        st.steps++;
        if (have) st.cur = c;
        if (a >= b) return have ? false : pop(st);
        if (have) { save(st, st.d, Frame{st.x, st.lo, st.hi, c}); st.d++; }
        st.x--; st.lo = a; st.hi = b;
        return enter(st);
    }
    GRL_DEV bool step(State &st) const { return step(st, FmNoTop{}); }
    GRL_DEV void end(u64 i, const State &st) const {
        if (!mism) { cnt[i] = st.cnt | (u64)st.cut << 63; return; }
        if (st.cnt != st.room) prim::atomic_max(bad, 1u);
        cnt[i] = st.steps;
    }
};
struct FmApproxLaneFn {   // the same, one lane per pattern through prim::top_search (GRLBWT_FM_MATCH=l)
    typedef FmKey Key;
    FmApproxFn f;
    GRL_HD const FmKey *keys() const { return f.keys(); }
    GRL_HD u64 n_keys() const { return f.n_keys(); }
    template <class TOP>
    GRL_DEV void operator()(u64 i, const TOP &top) const {
        FmApproxFn::State st;
        if (!f.begin(i, st)) return;
        while (!f.step(st, top)) {}                                      // (bounded as said above)
        f.end(i, st);
    }
};
struct FmApproxHitsIn {   // the count pass's word without its flag; the flag
    const u64 *cnt;
    GRL_DEV u64 operator()(u64 i) const { return cnt[i] & ~(1ull << 63); }
};
struct FmApproxCutIn {
    const u64 *cnt;
    GRL_DEV u64 operator()(u64 i) const { return cnt[i] >> 63; }
};
struct FmApproxMismIn {
    const u64 *mism; u64 d;
    GRL_DEV u64 operator()(u64 j) const { return mism[j] == d ? 1ull : 0ull; }
};
// ---- suffix-prefix overlaps (grlbwt_fm_overlaps / grlbwt_fm_overlaps_of / grlbwt_fm_overlap_targets).  Ticket i is
// query i.  A string starts with w exactly when the row of its whole-string suffix lies in the range of w, and the BWT symbol of
// that row is the separator: the strings that start with w are the separator ranks [rank_sep(lo), rank_sep(hi)), one more step
// with the separator as the symbol on a COPY of the range the backward search holds.  The separator is the smallest symbol, so
// C[sep] = 0 and the step's answer is the rank itself.  The ranks are the index of FmIndex::sid.  (A step bounded to the
// separator's records, key[0, Rsep), was measured against this plain one and dropped: under the LDS top level both searches
// start from one stride of the keys, and the bounded one was no faster -- profiles/fm_overlaps/overlaps.txt.)
//   The cells come from a source, last cell first and as codes: next() is false at the query's first cell, at the separator and
//   at a value that is no symbol (every longer suffix would hold it); whole() says that the cells taken so far are the whole
//   query.  FmOvCells reads the cells of a pattern, FmOvWalk the LF walk of a string of the collection (the walk of FmSidLenFn:
//   the index was made with the locate structures, so every string's walk has met the separator within n steps).
//   Two passes of this one search, as FmApproxFn: cnt[i] = hits while `olen` is null; then, with hoff = the scanned counts, the
//   entries in ascending L, cnt[i] = the pass's steps (below), and `bad` where a query found another number of hits than it had
//   counted.  The emit pass never stores past hoff[i + 1].
//   The emit pass's word: L << 2 | (the last query step emptied the range) << 1 | (L was the whole query under PROPER and had no
//   separator step), L = the cells matched.  Query steps = L + the second flag; separator steps = the L' in [floor, L] less
//   the first flag.
//   Loops: step() holds none but the binary searches; an item takes at most min(m, cap) + 1 steps of at most two fm_step each.
struct FmOvCells {
    struct State { u64 x0, x; };              // x cells are left
    FmCountFn f; u64 sepval;
    GRL_DEV void begin(u64 i, State &s) const { s.x0 = f.off[i]; s.x = f.off[i + 1] - s.x0; }
    GRL_DEV bool next(State &s, u32 &c) const {
        if (s.x == 0) return false;
        const u64 v = f.cell(s.x0 + s.x - 1);
        if (v == sepval || !f.code(v, c)) return false;
        s.x--;
        return true;
    }
    GRL_DEV bool whole(const State &s) const { return s.x == 0; }
};
struct FmOvWalk {
    struct State { idx_t row; RunRec r; };    // the row the walk stands at and its record
    LfRows lf; u32 sep; const u64 *ids;
    GRL_DEV void begin(u64 i, State &s) const { s.row = (idx_t)ids[i]; s.r = lf.at(s.row); }
    GRL_DEV bool next(State &s, u32 &c) const {
        if (s.r.sym == sep) return false;
        c = s.r.sym;
        s.row = LfRows::next(s.row, s.r);
        s.r = lf.at(s.row);
        return true;
    }
    GRL_DEV bool whole(const State &s) const { return s.r.sym == sep; }
};
template <class SRC>
struct FmOverlapFn {
    typedef FmKey Key;
    struct State { typename SRC::State s; u64 lo, hi, len, cnt, base, room; u32 flags; };
    SRC src;
    const FmKey *key; const idx_t *slf; u64 R, n; u32 sep;
    u64 floor, cap; bool proper;              // floor >= 1; cap: ~0 for none
    u64 *cnt; const u64 *hoff; u64 *olen, *tlo, *thi, *lo, *hi; u32 *bad;
    GRL_HD const FmKey *keys() const { return key; }
    GRL_HD u64 n_keys() const { return R; }
    GRL_DEV bool begin(u64 i, State &st) const {
        src.begin(i, st.s);
        st.lo = 0; st.hi = n; st.len = 0; st.cnt = 0; st.flags = 0;
        st.base = olen ? hoff[i] : 0; st.room = olen ? hoff[i + 1] - st.base : 0;
        if (st.lo >= st.hi) { end(i, st); return false; }                  // (an index of no symbol)
        return true;
    }
    template <class TOP>
    GRL_DEV bool step(State &st, const TOP &top) const {
        u32 c;
        if (!src.next(st.s, c)) return true;
        u64 a = st.lo, b = st.hi;
        fm_step(key, slf, R, top, c, a, b);
        if (a >= b) { st.flags |= 2u; return true; }
        st.lo = a; st.hi = b; st.len++;
        if (st.len >= floor) {
            if (proper && src.whole(st.s)) {
                st.flags |= 1u;
            } else {
                u64 ta = a, tb = b;
                fm_step(key, slf, R, top, sep, ta, tb);
                if (ta < tb) {
                    if (olen && st.cnt < st.room) {
                        const u64 j = st.base + st.cnt;
                        olen[j] = st.len; tlo[j] = ta; thi[j] = tb;
                        if (lo) { lo[j] = a; hi[j] = b; }
                    }
                    st.cnt++;
                }
            }
        }
        return st.len >= cap;
    }
    GRL_DEV bool step(State &st) const { return step(st, FmNoTop{}); }
    GRL_DEV void end(u64 i, const State &st) const {
        if (!olen) { cnt[i] = st.cnt; return; }
        if (st.cnt != st.room) prim::atomic_max(bad, 1u);
        cnt[i] = st.len << 2 | (u64)st.flags;
    }
};
template <class SRC>
struct FmOverlapLaneFn {  // the same, one lane per query through prim::top_search (GRLBWT_FM_MATCH=l)
    typedef FmKey Key;
    FmOverlapFn<SRC> f;
    GRL_HD const FmKey *keys() const { return f.keys(); }
    GRL_HD u64 n_keys() const { return f.n_keys(); }
    template <class TOP>
    GRL_DEV void operator()(u64 i, const TOP &top) const {
        typename FmOverlapFn<SRC>::State st;
        if (!f.begin(i, st)) return;
        while (!f.step(st, top)) {}                                      // (bounded as said above)
        f.end(i, st);
    }
};
struct FmOvQueryStepsIn { // the emit pass's word: the query steps; the separator steps
    const u64 *cnt;
    GRL_DEV u64 operator()(u64 i) const { return (cnt[i] >> 2) + ((cnt[i] >> 1) & 1ull); }
};
struct FmOvSepStepsIn {
    const u64 *cnt; u64 floor;
    GRL_DEV u64 operator()(u64 i) const {
        const u64 L = cnt[i] >> 2;
        return L >= floor ? L - floor + 1 - (cnt[i] & 1ull) : 0ull;
    }
};
struct FmOvIdBadIn {      // entry i when its string number is none, else ~0
    const u64 *ids; u64 k;
    GRL_DEV u64 operator()(u64 i) const { return ids[i] >= k ? i : ~0ull; }
};
struct FmOvRangeBadIn {   // range i when it is no range of prefix ranks, else ~0
    const u64 *tlo, *thi; u64 k;
    GRL_DEV u64 operator()(u64 i) const { return tlo[i] > thi[i] || thi[i] > k ? i : ~0ull; }
};
struct FmOvSpanIn {
    const u64 *tlo, *thi;
    GRL_DEV u64 operator()(u64 i) const { return thi[i] - tlo[i]; }
};
struct FmOvExpandFn {     // entry e of the expanded ranges through prim::for_each: the range that holds it by a search in the scanned offsets
    const u64 *eoff, *tlo; const idx_t *sid; u64 nr; u64 *str, *rng;
    GRL_DEV void operator()(u64 e) const {
        const u64 r = upper_bound<u64>(eoff, nr + 1, e) - 1;              // eoff[r] <= e < eoff[r + 1]: empty ranges are stepped over
        str[e] = (u64)sid[tlo[r] + (e - eoff[r])];
        if (rng) rng[e] = r;
    }
};
// sid: string i's walk (RunInvertLenFn's) ends at the row r that holds its separator; that separator is the LF(r)-th of the
// BWT.  The LF map of any image is a permutation, so a walk from one of the first k rows comes back to one of them after at
// most n steps; the bound is there for an index that is not what it should be.
struct FmSidLenFn {       // (slen, where an index extracts: the steps of string i's walk + the separator are its length; null: not wanted)
    LfRows lf; u32 sep; u64 n; idx_t *sid, *slen; u32 *bad;
    GRL_DEV void operator()(u64 i) const {
        idx_t row = (idx_t)i;
        u64 s = 0;
        RunRec r = lf.at(row);
        for (; s < n && r.sym != sep; s++) { row = LfRows::next(row, r); r = lf.at(row); }
        if (r.sym != sep) { prim::atomic_max(bad, 1u); return; }
        sid[(u64)LfRows::next(row, r)] = (idx_t)i;
        if (slen) slen[i] = (idx_t)(s + 1);
    }
};
struct FmRowBadIn {
    const u64 *rows; u64 n;
    GRL_DEV u64 operator()(u64 i) const { return rows[i] >= n ? 1ull : 0ull; }
};
struct FmLocateFn {       // row -> (string, offset): LF steps until the row's symbol is the separator, at most `lim` of them
    LfRows lf; const idx_t *sid; u32 sep; u64 lim; const u64 *rows; u64 *str, *ofs;
    GRL_DEV void operator()(u64 i) const {
        idx_t row = (idx_t)rows[i];
        u64 s = 0;
        RunRec r = lf.at(row);
        for (; s < lim && r.sym != sep; s++) { row = LfRows::next(row, r); r = lf.at(row); }
        const bool found = r.sym == sep;
        str[i] = found ? (u64)sid[(u64)LfRows::next(row, r)] : ~0ull;
        ofs[i] = found ? s : ~0ull;
    }
};

// ---- checkpointed LF walks.  The walks above run one lane per string, one dependent step per cell: their latency
// is the longest string.  Cut at CHECKPOINT rows they become m = k + ceil(n / s) segments of about s = 2^b steps, which a list
// ranking over the checkpoints puts back in order.  Rows [0, k) -- where the strings' walks start -- are checkpoints 0 .. k-1;
// every block of s rows [j s, (j + 1) s) holds one more, checkpoint k + j, at j s + (mix(j) & (s - 1)) (reduced modulo the length
// of the last, shorter block, so that every pick is a row).  A pick below k is void: that row is a head already.  LF is linear
// inside a run, so a plain stride would correlate with the walks of a repetitive text: the pick is jittered by a fixed 64-bit
// mixer.  Whether a row is a checkpoint, and which, is arithmetic: no array, no bit-vector.
struct Checkpoints {
    u64 n, k; u32 b;
    GRL_HD static u64 mix(u64 j) {                         // (splitmix64)
        u64 z = j + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    GRL_HD u64 blocks() const { return (n + (1ull << b) - 1) >> b; }
    GRL_HD u64 count() const { return k + blocks(); }
    GRL_HD u64 pick(u64 j) const {
        const u64 s = 1ull << b, base = j << b, len = n - base < s ? n - base : s;
        u64 off = mix(j) & (s - 1);
        if (off >= len) off %= len;
        return base + off;
    }
    GRL_HD u64 row_of(u64 c) const { return c < k ? c : pick(c - k); }
    GRL_HD bool is_void(u64 c) const { return c >= k && pick(c - k) < k; }
    GRL_HD u64 index_of(u64 row) const {                   // ~0: the row is no checkpoint (a row of [k, n) that is its block's pick is never void)
        if (row < k) return row;
        const u64 j = row >> b;
        return pick(j) == row ? k + j : ~0ull;
    }
};
static constexpr idx_t kCpNone = (idx_t)~(idx_t)0;        // no checkpoint / no string
static constexpr idx_t kCpEnd = (idx_t)(kCpNone - 1);     // next[]: the segment ends its string
// Phase A, one ticket per checkpoint c: LF steps from its row until the row reached is a checkpoint (next[c] = its number) or
// holds the separator (next[c] = kCpEnd, and endcp[slot] = c for the slot FmSidLenFn computes: that separator's row among [0, k)).
// seglen[c] = the steps.  A void checkpoint has next = none and no steps.  LF is a permutation and every row a walk starts at is a
// checkpoint, so a walk is back at a checkpoint after at most n steps: the bound is there for an index that is not what it should be.
struct CpSegFn {
    struct State { idx_t row; u64 steps; idx_t to; };
    LfRows lf; u32 sep; Checkpoints cp; idx_t *seglen, *next, *endcp; u32 *bad;
    GRL_DEV bool begin(u64 c, State &st) const {
        if (cp.is_void(c)) { seglen[c] = 0; next[c] = kCpNone; return false; }
        st.row = (idx_t)cp.row_of(c); st.steps = 0; st.to = kCpNone;
        return true;
    }
    GRL_DEV bool step(State &st) const {
        const RunRec r = lf.at(st.row);
        if (r.sym == sep) { st.to = kCpEnd; st.row = LfRows::next(st.row, r); return true; }
        st.row = LfRows::next(st.row, r);
        st.steps++;
        const u64 ci = cp.index_of((u64)st.row);
        if (ci != ~0ull) { st.to = (idx_t)ci; return true; }
        return st.steps >= cp.n;
    }
    GRL_DEV void end(u64 c, const State &st) const {
        seglen[c] = (idx_t)st.steps;
        next[c] = st.to;
        if (st.to == kCpEnd) endcp[(u64)st.row] = (idx_t)c;
        else if (st.to == kCpNone) prim::atomic_max(bad, 1u);
    }
};
// Phase B, list ranking by pointer jumping over prev.  ptr[c] = the checkpoint in front of c on its chain, acc[c] = the steps
// between them; a head points at itself with 0 steps, a checkpoint nobody reaches at nothing.
struct CpInitFn {
    u64 k; idx_t *ptr, *acc;
    GRL_DEV void operator()(u64 c) const { ptr[c] = c < k ? (idx_t)c : kCpNone; acc[c] = 0; }
};
struct CpPrevFn {         // prev[next[c]] = c: next is one-to-one (LF is a permutation), so every slot has one writer
    const idx_t *next, *seglen; idx_t *ptr, *acc;
    GRL_DEV void operator()(u64 c) const {
        const idx_t d = next[c];
        if (d == kCpNone || d == kCpEnd) return;
        ptr[(u64)d] = (idx_t)c; acc[(u64)d] = seglen[c];
    }
};
struct CpJumpFn {         // one round, from generation (p0, a0) to (p1, a1)
    const idx_t *p0, *a0; idx_t *p1, *a1;
    GRL_DEV void operator()(u64 c) const {
        const idx_t p = p0[c];
        if (p == kCpNone) { p1[c] = p; a1[c] = a0[c]; return; }
        const idx_t q = p0[(u64)p];
        p1[c] = q == kCpNone ? p : q;
        a1[c] = q == kCpNone ? a0[c] : (idx_t)(a0[c] + a0[(u64)p]);
    }
};
struct CpMovedIn {
    const idx_t *p0, *p1;
    GRL_DEV u64 operator()(u64 c) const { return p0[c] != p1[c] ? 1ull : 0ull; }
};
struct CpHeadFn {         // after the rounds: ptr[c] is c's string where it is a head, none elsewhere (a chain that is a cycle has none)
    u64 k; idx_t *ptr; u64 *chain;
    GRL_DEV void operator()(u64 c) const {
        const idx_t p = ptr[c];
        if (p != kCpNone && (u64)p >= k) ptr[c] = kCpNone;
        else if (p != kCpNone) prim::atomic_add(&chain[(u64)p], (u64)1);
    }
};
struct CpLenFn {          // string lengths from the chains' last checkpoints: dist + steps + the separator
    const idx_t *endcp, *head, *dist, *seglen; idx_t *slen; u32 *bad;
    GRL_DEV void operator()(u64 slot) const {
        const u64 e = (u64)endcp[slot];
        const idx_t h = head[e];
        if (h == kCpNone) { prim::atomic_max(bad, 1u); return; }
        slen[(u64)h] = (idx_t)(dist[e] + seglen[e] + 1);
    }
};
// Phase C of the inverter: phase A's walk again, every segment writing its cells backwards from the position its rank gives
template <class cell_t>
struct CpWriteFn {
    struct State { idx_t row; u64 pos, left; };
    LfRows lf; u32 sep; Checkpoints cp; const idx_t *head, *dist, *seglen, *off; cell_t *text; SymOut<cell_t> val;
    GRL_DEV bool begin(u64 c, State &st) const {
        const idx_t h = head[c];
        if (h == kCpNone) return false;
        st.row = (idx_t)cp.row_of(c);
        st.pos = (u64)off[(u64)h + 1] - 1 - (u64)dist[c];
        st.left = (u64)seglen[c];
        if (c < cp.k) text[st.pos] = val(sep);
        return st.left != 0;
    }
    GRL_DEV bool step(State &st) const {
        const RunRec r = lf.at(st.row);
        text[--st.pos] = val(r.sym);
        st.row = LfRows::next(st.row, r);
        return --st.left == 0;
    }
    GRL_DEV void end(u64, const State &) const {}
};
// The store form of the write walk for u8 / u16 cells into an 8-byte aligned text (CpWriteFn otherwise): the cells of one aligned
// 8-byte word of the text are collected in a register and stored as that word.  A segment's first and last word are shared with its neighbours' segments: what a lane holds of
// a word it does not own whole goes out cell by cell.  [pos, top) is what the register holds; it never crosses a word.
template <class cell_t>
struct CpWritePackedFn {
    static constexpr u64 kPer = 8 / sizeof(cell_t), kBits = 8 * sizeof(cell_t);
    struct State { idx_t row; u64 pos, left, top, acc; };
    CpWriteFn<cell_t> w;
    GRL_DEV bool begin(u64 c, State &st) const {
        typename CpWriteFn<cell_t>::State s;
        const bool go = w.begin(c, s);
        st.row = s.row; st.pos = s.pos; st.left = s.left; st.top = s.pos; st.acc = 0;
        return go;
    }
    GRL_DEV bool step(State &st) const {
        const RunRec r = w.lf.at(st.row);
        --st.pos;
        st.acc |= (u64)w.val(r.sym) << ((st.pos & (kPer - 1)) * kBits);
        st.row = LfRows::next(st.row, r);
        --st.left;
        const bool bottom = (st.pos & (kPer - 1)) == 0;
        if (bottom || st.left == 0) {
            if (bottom && st.top - st.pos == kPer) *reinterpret_cast<u64 *>(w.text + st.pos) = st.acc;
            else for (u64 q = st.pos; q < st.top; q++) w.text[q] = (cell_t)(st.acc >> ((q & (kPer - 1)) * kBits));      // (fewer than kPer cells)
            st.top = st.pos; st.acc = 0;
        }
        return st.left == 0;
    }
    GRL_DEV void end(u64, const State &) const {}
};
template <class F>
struct WalkSerialFn {     // the serial form of prim::walk_tickets: one item after the other through prim::for_each
    F f;
    GRL_DEV void operator()(u64 c) const {
        typename F::State st;
        if (!f.begin(c, st)) return;
        while (!f.step(st)) {}
        f.end(c, st);
    }
};
// Phase C of the index: the string behind every separator from the chain ends, and per checkpoint the sample (string, offset of
// the row's suffix in it)
struct CpSidFn {
    const idx_t *endcp, *head; idx_t *sid;
    GRL_DEV void operator()(u64 slot) const { sid[slot] = head[(u64)endcp[slot]]; }
};
struct CpSampleFn {
    const idx_t *head, *dist, *slen; idx_t *smp;
    GRL_DEV void operator()(u64 c) const {
        const idx_t h = head[c];
        smp[2 * c] = h;
        smp[2 * c + 1] = h == kCpNone ? kCpNone : (idx_t)(slen[(u64)h] - 1 - dist[c]);
    }
};
// locate over an index with samples: the walk also stops at a checkpoint row; one met after t steps gives (string, offset + t).
// A checkpoint without a string lies on a cycle of rows that holds no separator: the row has no position, as in FmLocateFn, whose
// walk runs into its bound.  An offset above `lim` is suppressed: the contract is FmLocateFn's.
struct FmLocateCpFn {
    LfRows lf; const idx_t *sid, *smp; Checkpoints cp; u32 sep; u64 lim; const u64 *rows; u64 *str, *ofs;
    GRL_DEV void operator()(u64 i) const {
        idx_t row = (idx_t)rows[i];
        u64 rs = ~0ull, ro = ~0ull;
        for (u64 s = 0; s <= lim; s++) {
            const u64 ci = cp.index_of((u64)row);
            if (ci != ~0ull) {
                const idx_t h = smp[2 * ci];
                if (h != kCpNone) { const u64 o = (u64)smp[2 * ci + 1] + s; if (o <= lim) { rs = (u64)h; ro = o; } }
                break;
            }
            const RunRec r = lf.at(row);
            if (r.sym == sep) { rs = (u64)sid[(u64)LfRows::next(row, r)]; ro = s; break; }
            row = LfRows::next(row, r);
        }
        str[i] = rs; ofs[i] = ro;
    }
};

// ---- the document array and the suffix array (grlbwt_fm_sa): FmLocateFn's answer for EVERY row.  A locate walks
// each row to its string's start or to a checkpoint on its own; the LF chain of a string visits each of its rows once, so a walk per
// string -- or per checkpoint segment -- that stores (string, offset) at every row it passes writes both arrays in n steps.  A row
// lies on one chain, and on it is either a checkpoint or interior to one segment: one writer per entry, no atomics.
template <int W> struct SaCell;
template <> struct SaCell<1> { typedef u8 type; };
template <> struct SaCell<2> { typedef u16 type; };
template <> struct SaCell<4> { typedef u32 type; };
template <> struct SaCell<8> { typedef u64 type; };
template <int W> struct SaOut {      // one output of W bytes per entry
    typename SaCell<W>::type *p;
    GRL_DEV void put(u64 i, u64 v) const { p[i] = (typename SaCell<W>::type)v; }
};
template <> struct SaOut<0> {        // the output was not asked for: no store, no branch
    GRL_DEV void put(u64, u64) const {}
};
struct SaWindow {                    // the rows [lo, lo + len) are stored at entry row - lo, the others are walked only
    u64 lo, len;
    GRL_DEV bool holds(idx_t row, u64 &at) const { at = (u64)row - lo; return at < len; }      // (wraps below lo)
};
struct SaLenFn {          // the length pass of form 0 (FmSidLenFn's walk, as tickets): slen[i] = the steps of string i's walk + the separator
    struct State { idx_t row; u64 steps; };
    LfRows lf; u32 sep; u64 n; idx_t *slen;
    GRL_DEV bool begin(u64 i, State &st) const { st.row = (idx_t)i; st.steps = 0; return true; }
    GRL_DEV bool step(State &st) const {
        const RunRec r = lf.at(st.row);
        if (r.sym == sep) return true;
        st.row = LfRows::next(st.row, r);
        return ++st.steps >= n;              // (an index with the locate structures has walks that end: FmSidLenFn)
    }
    GRL_DEV void end(u64 i, const State &st) const { slen[i] = (idx_t)(st.steps + 1); }
};
// Form 0, one ticket per string i: from row i, whose suffix is the separator alone at offset slen[i] - 1, store and step until the
// row whose symbol is the separator -- offset 0 -- has been stored.  slen is read only where offsets are written.
template <int WS, int WO>
struct SaStringFn {
    struct State { idx_t row; u64 str, ofs, steps; };
    LfRows lf; u32 sep; u64 n; const idx_t *slen; SaWindow win; SaOut<WS> so; SaOut<WO> oo; idx_t *wsteps;
    GRL_DEV bool begin(u64 i, State &st) const {
        st.row = (idx_t)i; st.str = i; st.steps = 0; st.ofs = 0;
        if constexpr (WO != 0) st.ofs = (u64)slen[i] - 1;
        return true;
    }
    GRL_DEV bool step(State &st) const {
        u64 at;
        if (win.holds(st.row, at)) { so.put(at, st.str); oo.put(at, st.ofs); }
        const RunRec r = lf.at(st.row);
        if (r.sym == sep) return true;
        st.row = LfRows::next(st.row, r);
        st.ofs--;
        return ++st.steps >= n;
    }
    GRL_DEV void end(u64 i, const State &st) const { wsteps[i] = (idx_t)st.steps; }
};
// Form 1, one ticket per checkpoint c (CpSegFn's walk with stores): from the checkpoint's row with its kept sample, store and step
// until the separator's row has been stored or the row reached is a checkpoint -- that row is another ticket's.  A void checkpoint
// and one on no string's chain have no sample and no walk.
template <int WS, int WO>
struct SaSegFn {
    struct State { idx_t row; u64 str, ofs, steps; };
    LfRows lf; u32 sep; Checkpoints cp; const idx_t *smp; SaWindow win; SaOut<WS> so; SaOut<WO> oo; idx_t *wsteps;
    GRL_DEV bool begin(u64 c, State &st) const {
        const idx_t h = smp[2 * c];
        if (h == kCpNone) { wsteps[c] = 0; return false; }
        st.row = (idx_t)cp.row_of(c); st.str = (u64)h; st.ofs = (u64)smp[2 * c + 1]; st.steps = 0;
        return true;
    }
    GRL_DEV bool step(State &st) const {
        u64 at;
        if (win.holds(st.row, at)) { so.put(at, st.str); oo.put(at, st.ofs); }
        const RunRec r = lf.at(st.row);
        if (r.sym == sep) return true;
        st.row = LfRows::next(st.row, r);
        st.ofs--;
        st.steps++;
        return cp.index_of((u64)st.row) != ~0ull || st.steps >= cp.n;
    }
    GRL_DEV void end(u64 c, const State &st) const { wsteps[c] = (idx_t)st.steps; }
};
struct SaHeadLenIn {      // the length of string i, separator included, from its head's sample (0: the head is on no chain -- never, a head starts one)
    const idx_t *smp;
    GRL_DEV u64 operator()(u64 i) const { return smp[2 * i] == kCpNone ? 0ull : (u64)smp[2 * i + 1] + 1; }
};
struct SaStartLenFn {     // the same from the strings' start positions of an index that extracts
    const idx_t *T; idx_t *slen;
    GRL_DEV void operator()(u64 i) const { slen[i] = (idx_t)(T[i + 1] - T[i]); }
};

// ---- the strings behind row ranges (grlbwt_docs_*).  DA[p] is the string of row p, PREV[p] the largest row below p
// with the same string (kCpNone: there is none), LST the rows sorted by (string, row) and START[d] where string d's rows begin in
// LST.  Row p of a range [lo, hi) is the first row of its string in the range exactly when PREV[p] is none or below lo: the
// documents of a range are the set bits of that test over its rows, in ascending row.  The rows of all ranges of a batch are
// laid back to back, range r at [roff[r], roff[r + 1]): position x of that sequence is row lo[r] + (x - roff[r]) of the range
// r that holds it, and one bit per position with its word ranks gives every range its count and every document its entry.
//   Bounds: x < roff[nr] lies in a range r that is not empty, so its row is below hi[r] <= n (the caller has checked the ranges);
//   DA of a row is below k (the create refuses an image whose chains miss a row), so START[d + 1] is defined; a rank is read at
//   position x <= roff[nr], word x / 64 of roff[nr] / 64 + 2 zeroed words.
struct DocsIotaFn {          // the sort's input: the string as the key, the row as the value
    const idx_t *da; idx_t *key, *val;
    GRL_DEV void operator()(u64 p) const { key[p] = da[p]; val[p] = (idx_t)p; }
};
struct DocsPrevFn {          // one writer per row: LST is a permutation of the rows
    const idx_t *key, *lst; idx_t *prev;
    GRL_DEV void operator()(u64 i) const { prev[lst[i]] = (i > 0 && key[i] == key[i - 1]) ? lst[i - 1] : kCpNone; }
};
struct DocsStartFn {         // one writer per string (every string owns its terminator's row), and the end
    const idx_t *key; u64 n, k; idx_t *start;
    GRL_DEV void operator()(u64 i) const {
        if (i == n) { start[k] = (idx_t)n; return; }
        if (i == 0 || key[i] != key[i - 1]) start[key[i]] = (idx_t)i;
    }
};
struct DocsRangeBadIn {      // range r when it is no range of rows, else ~0
    const u64 *lo, *hi; u64 n;
    GRL_DEV u64 operator()(u64 r) const { return lo[r] > hi[r] || hi[r] > n ? r : ~0ull; }
};
struct DocsSpanIn {
    const u64 *lo, *hi;
    GRL_DEV u64 operator()(u64 r) const { return hi[r] - lo[r]; }
};
struct DocsFirstPred {       // the generic form of the flags: a search per range row
    const u64 *roff, *lo; const idx_t *prev; u64 nr;
    GRL_DEV bool operator()(u64 x) const {
        const u64 r = upper_bound<u64>(roff, nr + 1, x) - 1;              // roff[r] <= x < roff[r + 1]: empty ranges are stepped over
        const idx_t v = prev[lo[r] + (x - roff[r])];
        return v == kCpNone || (u64)v < lo[r];
    }
};
struct DocsRank {            // set bits in front of position x
    const u64 *words, *wrank;
    GRL_DEV u64 operator()(u64 x) const { return wrank[x >> 6] + (u64)__builtin_popcountll(words[x >> 6] & ((1ull << (x & 63)) - 1ull)); }
};
struct DocsCountIn {         // the documents of range r
    const u64 *roff; DocsRank rk;
    GRL_DEV u64 operator()(u64 r) const { return rk(roff[r + 1]) - rk(roff[r]); }
};
struct DocsCountFn {
    DocsCountIn in; u64 *ndocs;
    GRL_DEV void operator()(u64 r) const { ndocs[r] = in(r); }
};
struct DocsOffsetFn {        // entry_offsets[r], r = 0 .. nr
    const u64 *roff; DocsRank rk; u64 *eoff;
    GRL_DEV void operator()(u64 r) const { eoff[r] = rk(roff[r]); }
};
struct DocsOcc {             // the rows of string d in [first, hi): two searches in d's part of LST (null LST: not asked for)
    const idx_t *lst, *start;
    GRL_DEV u64 operator()(u64 d, u64 first, u64 hi) const {
        const u64 a = (u64)start[d], m = (u64)start[d + 1] - a;
        const u64 top = hi > (u64)kCpNone ? (u64)kCpNone : hi;             // (rows are below kCpNone)
        return lower_bound<idx_t>(lst + a, m, (idx_t)top) - lower_bound<idx_t>(lst + a, m, (idx_t)first);
    }
};
struct DocsEmitFn {          // the generic form of the entries, prim::for_each_set_bit over the flags: a search per entry
    const u64 *roff, *lo, *hi; const idx_t *da; DocsOcc oc; u64 nr; u64 *str, *frow, *occ, *rng;
    GRL_DEV void operator()(u64 x, u64 e) const {
        const u64 r = upper_bound<u64>(roff, nr + 1, x) - 1;
        const u64 p = lo[r] + (x - roff[r]), d = (u64)da[p];
        str[e] = d;
        if (frow) frow[e] = p;
        if (occ) occ[e] = oc(d, p, hi[r]);
        if (rng) rng[e] = r;
    }
};

// ---- removing or keeping chosen strings (grlbwt_select_*).  The suffixes of string i are the rows on the LF chain
// from row i to the row whose symbol is the separator; the chains of distinct strings are disjoint.  The walks set one bit per
// chain row of the LISTED strings; the rows a run loses (or keeps) are then a difference of two ranks over those bits.
struct SelListFn {        // the list as a set: bit s of a k-bit vector for every entry s
    const u64 *ids; u64 *bits;
    GRL_DEV void operator()(u64 i) const { const u64 s = ids[i]; prim::atomic_or(&bits[s >> 6], 1ull << (s & 63)); }
};
struct SelTicketFn {      // prim::for_each_set_bit over that vector: the distinct entries in ascending order
    idx_t *tick;
    GRL_DEV void operator()(u64 p, u64 ord) const { tick[ord] = (idx_t)p; }
};
GRL_DEV bool sel_listed(const u64 *bits, u64 s) { return (bits[s >> 6] >> (s & 63)) & 1ull; }
// (several lanes share a word, hence the atomic; a row lies on one chain, so no bit is set twice, and nothing reads the result)
GRL_DEV void sel_mark(u64 *mark, u64 row) { prim::atomic_or(&mark[row >> 6], 1ull << (row & 63)); }
// Marking per string, one ticket per listed string: row = its number, then LF steps up to and including the row whose symbol is
// the separator.  As in FmSidLenFn a walk from one of the first k rows meets that row after at most n steps whatever the image is;
// the bound is there all the same.  steps[t] = the rows marked = the string's length, separator included.
struct SelMarkFn {
    struct State { idx_t row; u64 steps; bool found; };
    LfRows lf; u32 sep; u64 n; const idx_t *tick; u64 *mark; idx_t *steps; u32 *bad;
    GRL_DEV bool begin(u64 t, State &st) const { st.row = tick[t]; st.steps = 0; st.found = false; return true; }
    GRL_DEV bool step(State &st) const {
        sel_mark(mark, (u64)st.row);
        const RunRec r = lf.at(st.row);
        st.steps++;
        if (r.sym == sep) { st.found = true; return true; }
        st.row = LfRows::next(st.row, r);
        return st.steps >= n;
    }
    GRL_DEV void end(u64 t, const State &st) const {
        steps[t] = (idx_t)st.steps;
        if (!st.found) prim::atomic_max(bad, 1u);
    }
};
// Marking through checkpointed segments, one ticket per checkpoint (CpWriteFn's shape): the segments of listed strings mark
// their seglen rows.  The row a segment ends at is either the next checkpoint's (that segment marks it) or the row whose symbol
// is the separator, which CpSegFn does not count: the last step looks at that row and marks it where it holds the separator.  (A
// checkpoint row that holds the separator is marked from both sides, by segments of the same string.)
struct SelMarkCpFn {
    struct State { idx_t row; u64 left; };
    LfRows lf; u32 sep; Checkpoints cp; const idx_t *head, *seglen; const u64 *list; u64 *mark;
    GRL_DEV bool begin(u64 c, State &st) const {
        const idx_t h = head[c];
        if (h == kCpNone || !sel_listed(list, (u64)h)) return false;
        st.row = (idx_t)cp.row_of(c);
        st.left = (u64)seglen[c];
        return true;
    }
    GRL_DEV bool step(State &st) const {
        const RunRec r = lf.at(st.row);
        if (st.left == 0) {
            if (r.sym == sep) sel_mark(mark, (u64)st.row);
            return true;
        }
        sel_mark(mark, (u64)st.row);
        st.row = LfRows::next(st.row, r);
        st.left--;
        return false;
    }
    GRL_DEV void end(u64, const State &) const {}
};
struct SelListedLenIn {   // the length of the t-th listed string (CpLenFn's slen)
    const idx_t *tick, *slen;
    GRL_DEV u64 operator()(u64 t) const { return (u64)slen[(u64)tick[t]]; }
};
struct SelSegStepsIn {    // the steps of checkpoint c's marking walk (0: not walked)
    const idx_t *head, *seglen; const u64 *list;
    GRL_DEV u64 operator()(u64 c) const {
        const idx_t h = head[c];
        return h != kCpNone && sel_listed(list, (u64)h) ? (u64)seglen[c] : 0ull;
    }
};
struct SelRunLenFn {      // the rewrite: a run's length less the marked rows in it -- or those alone, to keep the listed strings
    const idx_t *rpos; const u64 *mark; const idx_t *mbase; bool keep; idx_t *len;
    GRL_DEV void operator()(u64 r) const {
        const u64 a = (u64)rpos[r], b = (u64)rpos[r + 1], cnt = rank1(mark, mbase, b) - rank1(mark, mbase, a);
        len[r] = (idx_t)(keep ? cnt : (b - a) - cnt);
    }
};

// ---- extracting text ranges (grlbwt_fm_extract).  T[s] = the cells in front of string s, so (s, o) is the absolute
// position T[s] + o.  The index keeps the INVERSE of its samples: xq = the absolute positions of the sampled rows, ascending, and
// xc = the checkpoint of each (its row is cp.row_of).  The head of string s is a sample at T[s + 1] - 1, its separator's position,
// so every cell of a string lies below a sample of that string, and one LF step from the row of position x reads cell x - 1.
struct FmHeadSampleFn {   // without checkpoints the samples are the k heads: sorted as they come
    const idx_t *T; idx_t *xq, *xc;
    GRL_DEV void operator()(u64 s) const { xq[s] = (idx_t)(T[s + 1] - 1); xc[s] = (idx_t)s; }
};
struct FmCpSampleKeyFn {  // checkpoint c -> (absolute position, c); n, above every position, for a void checkpoint or one on no string's chain
    Checkpoints cp; const idx_t *head, *dist, *T; idx_t *key, *val;
    GRL_DEV void operator()(u64 c) const {
        const idx_t h = head[c];
        const bool has = h != kCpNone && !cp.is_void(c);
        key[c] = has ? (idx_t)(T[(u64)h + 1] - 1 - dist[c]) : (idx_t)cp.n;
        val[c] = (idx_t)c;
    }
};
struct FmSampleValidIn {
    const idx_t *key; u64 n;
    GRL_DEV u64 operator()(u64 c) const { return (u64)key[c] != n ? 1ull : 0ull; }
};
struct FmLenOutFn {
    const idx_t *T; u64 *len;
    GRL_DEV void operator()(u64 s) const { len[s] = (u64)T[s + 1] - (u64)T[s]; }
};
struct FmExtractBadIn {   // the number of a range whose string is none, else ~0
    const u64 *str; u64 k;
    GRL_DEV u64 operator()(u64 i) const { return str[i] >= k ? i : ~0ull; }
};
// Range i of string s = str[i]: cells [b, e) with e clamped to the string's length, [B, E) in absolute positions.  The separator's
// cell (E = T[s + 1]) is stored directly, the cells [B, E') in front of it are walked: E' = E - 1 there, E elsewhere.
struct FmRange {
    u64 B, E, Ew;         // Ew = E': (B < Ew: there is something to walk)
    bool sep;
};
struct FmExtractPlan {
    const idx_t *T, *xq; u64 ns; const u64 *str, *beg, *end;
    GRL_DEV FmRange range(u64 i) const {
        const u64 s = str[i], t0 = (u64)T[s], t1 = (u64)T[s + 1], len = t1 - t0;
        const u64 e = end[i] < len ? end[i] : len, b = beg[i] < e ? beg[i] : e;      // (b >= e: empty)
        FmRange r;
        r.B = t0 + b; r.E = t0 + e;
        r.sep = b < e && r.E == t1;
        r.Ew = r.sep ? r.E - 1 : r.E;
        return r;
    }
    GRL_DEV u64 first_above(u64 B) const { return upper_bound<idx_t>(xq, ns, (idx_t)B); }       // the first sample q > B
};
// The pieces of a range are the samples q with B < q <= q_top, q_top = the smallest sample >= E' (it exists, in the same string:
// the head); cells = its length; steps = the cells walked + the steps q_top - E' its top piece takes before it writes.
struct FmExtractPlanFn {
    FmExtractPlan p; u64 *npiece, *ncell, *nstep;
    GRL_DEV void operator()(u64 i) const {
        const FmRange r = p.range(i);
        u64 pieces = 0, steps = 0;
        if (r.B < r.Ew) {
            const u64 top = lower_bound<idx_t>(p.xq, p.ns, (idx_t)r.Ew);
            pieces = top - p.first_above(r.B) + 1;
            steps = (u64)p.xq[top] - r.B;
        }
        npiece[i] = pieces; ncell[i] = r.E - r.B; nstep[i] = steps;
    }
};
template <class cell_t>
struct FmExtractSepFn {   // the separator of every range that reaches its string's end
    FmExtractPlan p; const u64 *ooff; cell_t *out; cell_t sepval;
    GRL_DEV void operator()(u64 i) const {
        const FmRange r = p.range(i);
        if (r.sep) out[ooff[i] + (r.E - r.B) - 1] = sepval;
    }
};
// One ticket per piece.  Piece j of range i (pscan[i] <= ticket < pscan[i + 1]) belongs to sample first_above(B) + j, at position
// q; it writes the cells [lo, top), lo = B for j = 0 and the sample below q otherwise, top = min(q, E'), walking backwards from
// q's row: q - top steps that store nothing (the top piece alone has any), then one store per step.
//   Bounds, known before the launch: the steps of a piece are q - lo <= the gap between neighbouring samples <= n, and lo >= T[s]:
//   the walk never steps from its string's first row.  A cell x of range i goes to ooff[i] + (x - B) < ooff[i + 1] <= n_cells, which
//   the caller has checked against the capacity.
template <class cell_t>
struct FmExtractFn {
    struct State { idx_t row; u64 skip, left, o; };
    LfRows lf; Checkpoints cp; const idx_t *xc; FmExtractPlan p; u64 nr; const u64 *pscan, *ooff; cell_t *out; SymOut<cell_t> val;
    GRL_DEV bool begin(u64 t, State &st) const {
        const u64 i = upper_bound<u64>(pscan, nr + 1, t) - 1;       // (ranges without a piece are stepped over)
        const u64 j = t - pscan[i];
        const FmRange r = p.range(i);
        const u64 x = p.first_above(r.B) + j;
        const u64 q = (u64)p.xq[x], lo = j ? (u64)p.xq[x - 1] : r.B, top = q < r.Ew ? q : r.Ew;
        st.row = (idx_t)cp.row_of((u64)xc[x]);
        st.skip = q - top; st.left = top - lo;
        st.o = ooff[i] + (top - r.B);
        return true;                                                // (left >= 1: lo < top by the choice of the samples)
    }
    GRL_DEV bool step(State &st) const {
        const RunRec r = lf.at(st.row);
        st.row = LfRows::next(st.row, r);
        if (st.skip) { st.skip--; return false; }
        out[--st.o] = val(r.sym);
        return --st.left == 0;
    }
    GRL_DEV void end(u64, const State &) const {}
};

// ---- the LCP array of the collection (grlbwt_fm_lcp).  B holds one bit per row: set once the row's suffix is
// known to differ from the suffix of the row above within the first l cells.  A pass reads the rows in F-order: row q >= k lies
// in the sorted run j with slf[j] <= q < slf[j + 1] (one bit per slf[j], with ranks: frc) and is LF of row p = key[j].start() +
// (q - slf[j]); row q - 1 is LF of the occurrence of the same symbol in front of p, so the two suffixes differ within l + 1 cells
// when any row between the two occurrences (the later one included) differs from its predecessor within l.  Inside a run that
// is B[p] alone; at a run's first row it is a rank difference over B, from the end of the run in front.  S holds the rows whose
// suffix has exactly l cells: S'[q] = S[p].
//   Bounds: q < n gives j < R (frc has a bit at slf[0] = 0) and p inside run j, so p < n; q >= k gives j >= 1, since the runs of
//   the separator, the smallest symbol, cover rows [0, k); pe = the end of run j - 1 <= p when both hold one symbol, since the
//   sorted order of one symbol's runs is their order in the BWT.  rank1 reads word (p + 1) / 64 <= n / 64 of n / 64 + 2.
GRL_DEV bool lcp_bit(const u64 *w, u64 p) { return ((w[p >> 6] >> (p & 63)) & 1ull) != 0; }
struct LcpRowFn {
    const RankCell *frc; const FmKey *key; const idx_t *slf; u64 k;
    const u64 *B; const idx_t *brank; const u64 *S;
    GRL_DEV u64 run(u64 q) const { return run_of_row(frc, q); }
    // (single exit everywhere: the rows of a wave take different branches)
    GRL_DEV bool head(u64 q) const {          // before the first pass: the first row of a symbol, and every terminator
        bool h = true;
        if (q >= k) {
            const u64 j = run(q);
            h = q == (u64)slf[j] && (j == 0 || key[j].sym() != key[j - 1].sym());
        }
        return h;
    }
    // the row's bit of B' (bq: its bit of B) and of S'
    GRL_DEV bool operator()(u64 q, bool bq, bool &s) const {
        bool b = true;
        s = false;
        if (q >= k) {
            const u64 j = run(q);
            const FmKey kj = key[j];
            const u64 f = (u64)slf[j], p = kj.start() + (q - f);
            s = lcp_bit(S, p);
            b = bq;
            if (!b) {
                if (q > f) {
                    b = lcp_bit(B, p);
                } else if (j == 0) {
                    b = true;
                } else {
                    const FmKey kp = key[j - 1];
                    const u64 pe = kp.start() + (f - (u64)slf[j - 1]);
                    b = kp.sym() != kj.sym() || rank1(B, brank, p + 1) != rank1(B, brank, pe);
                }
            }
        }
        return b;
    }
    GRL_DEV bool len(u64 q) const {
        bool s = false;
        if (q >= k) {
            const u64 j = run(q);
            s = lcp_bit(S, key[j].start() + (q - (u64)slf[j]));
        }
        return s;
    }
};
struct LcpHeadPred {
    LcpRowFn f;
    GRL_DEV bool operator()(u64 q) const { return f.head(q); }
};
struct LcpBelowPred {       // S_0: the terminator-only suffixes
    u64 k;
    GRL_DEV bool operator()(u64 q) const { return q < k; }
};
struct LcpPassPred {        // the generic form of a pass: B' ...
    LcpRowFn f;
    GRL_DEV bool operator()(u64 q) const { bool s; return f(q, lcp_bit(f.B, q), s); }
};
struct LcpLenPred {         // ... and S'
    LcpRowFn f;
    GRL_DEV bool operator()(u64 q) const { return f.len(q); }
};
struct LcpNewFn {           // old := the bits of cur that old lacks
    const u64 *cur; u64 *old;
    GRL_DEV void operator()(u64 i) const { old[i] = cur[i] & ~old[i]; }
};
struct LcpUnsetPred {
    const u64 *B;
    GRL_DEV bool operator()(u64 q) const { return !lcp_bit(B, q); }
};
struct LcpStoreFn {         // prim::for_each_set_bit: the value v, in the output's width, at every set row
    void *out; int w; u64 v;
    GRL_DEV void operator()(u64 p, u64) const {
        switch (w) {
            case 1: ((u8 *)out)[p] = (u8)v; break;
            case 2: ((u16 *)out)[p] = (u16)v; break;
            case 4: ((u32 *)out)[p] = (u32)v; break;
            default: ((u64 *)out)[p] = v; break;
        }
    }
};

// ---- the distinct k-mers with their counts (grlbwt_fm_kmers).  After the LCP passes capped at k, B marks the rows
// with LCP < k: the boundaries of the k-mer intervals.  A boundary whose suffix has fewer than k cells heads no k-mer (Short, the
// OR of the generations of S up to k - 1), so the heads are H = B & ~Short and count(p) is the distance from head p to the next
// bit of B, or to n.  That next bit is in p's own word or in the next non-empty word of B: NZ holds one bit per non-empty word,
// with ranks, and nzlist the non-empty words in ascending order -- O(1) per head whatever the gap, no scan over it.
//   Bounds: p < n is a set bit of B, so word p / 64 is non-empty and its rank r in NZ has nzlist[r] = p / 64; r + 1 < nnz is
//   tested before nzlist[r + 1] is read, and that word is non-empty: ctz is defined.  B has no bit at or behind n.
struct KmerOrFn {            // acc |= cur, word by word
    const u64 *cur; u64 *acc;
    GRL_DEV void operator()(u64 i) const { acc[i] |= cur[i]; }
};
struct KmerHeadsFn {         // H = B & ~Short
    const u64 *B; const u64 *sh; u64 *H;
    GRL_DEV void operator()(u64 i) const { H[i] = B[i] & ~sh[i]; }
};
struct KmerWordPred {        // NZ: the words of B that hold a bit
    const u64 *B;
    GRL_DEV bool operator()(u64 w) const { return B[w] != 0; }
};
struct KmerWordListFn {      // prim::for_each_set_bit over NZ: the r-th non-empty word
    idx_t *nzlist;
    GRL_DEV void operator()(u64 w, u64 r) const { nzlist[r] = (idx_t)w; }
};
struct KmerCountFn {         // count(p) of a head p
    const u64 *B; const u64 *NZ; const idx_t *nzbase; const idx_t *nzlist; u64 nnz, n;
    GRL_DEV u64 operator()(u64 p) const {
        const u64 w = p >> 6;
        const u64 rest = (B[w] >> (p & 63)) >> 1;
        u64 nx = n;
        if (rest) {
            nx = p + 1 + (u64)__builtin_ctzll(rest);
        } else {
            const u64 r = (u64)nzbase[w >> 6] + (u64)__builtin_popcountll(NZ[w >> 6] & ((1ull << (w & 63)) - 1ull)) + 1;
            if (r < nnz) { const u64 x = (u64)nzlist[r]; nx = x * 64 + (u64)__builtin_ctzll(B[x]); }
        }
        return nx - p;
    }
};
struct KmerFilter {          // the table's rows: row_begin <= lo < row_end, cmin <= count <= cmax
    u64 rb, re, cmin, cmax;
    GRL_DEV bool operator()(u64 p, u64 c) const { return p >= rb && p < re && c >= cmin && c <= cmax; }
};
struct KmerSelPred {
    const u64 *H; KmerCountFn cnt; KmerFilter flt;
    GRL_DEV bool operator()(u64 p) const { return lcp_bit(H, p) && flt(p, cnt(p)); }
};
struct KmerWindowsIn {       // count(p) at a head, 0 elsewhere: their sum is the number of windows, their maximum the largest count
    const u64 *H; KmerCountFn cnt;
    GRL_DEV u64 operator()(u64 p) const { return lcp_bit(H, p) ? cnt(p) : 0ull; }
};
struct KmerSpectrumFn {      // the serial form of the spectrum: prim::for_each_set_bit over H (the device form: prim::kmer_spectrum)
    KmerCountFn cnt; u64 *bins; u64 last;
    GRL_DEV void operator()(u64 p, u64) const { const u64 c = cnt(p); prim::atomic_add(&bins[c < last ? c : last], (u64)1); }
};
// The forward step: row q >= n_strings lies in sorted run j, its suffix starts with key[j].sym() and goes on with the suffix of
// row key[j].start() + (q - slf[j]).  q < n gives j < R and a row inside run j, so the next q is below n again: the walk reads in
// bounds on any image, and on the BWT of a collection a head's k steps stay at rows >= n_strings (its suffix has k cells).
struct KmerStepFn {
    const RankCell *frc; const FmKey *key; const idx_t *slf; const u64 *alpha;
    GRL_DEV u64 operator()(u64 &q) const {
        const u64 j = run_of_row(frc, q);
        const FmKey kj = key[j];
        q = kj.start() + (q - (u64)slf[j]);
        const u64 c = (u64)kj.sym();
        return alpha ? alpha[c] : c;
    }
};
template <class cell_t>
struct KmerEmitFn {          // the generic decode, prim::for_each_set_bit over the selected bits: one lane per entry stores its own cells
    KmerStepFn step; KmerCountFn cnt; u64 k; cell_t *cells; u64 *lo; u64 *count;
    GRL_DEV void operator()(u64 p, u64 e) const {
        if (lo) lo[e] = p;
        if (count) count[e] = cnt(p);
        if (cells) {
            u64 q = p;
            for (u64 t = 0; t < k; t++) cells[e * k + t] = (cell_t)step(q);
        }
    }
};

// ---- the strand-merged k-mers (grlbwt_fm_kmers_canonical).  The reverse complement of the k-mer x of head p is
// found without its cells being stored anywhere: the forward walk from p yields x_0, x_1, ... and the backward search for
// rc(x) = comp(x_{k-1}) ... comp(x_0) consumes its pattern from the last cell, comp(x_0), onward -- the same order -- so one item
// alternates a forward step (KmerStepFn's, here for the symbol CODE) with one fm_step on a range that starts at [0, n).
//   mate[e] of the head with rank e: the head row of rc(x) when it occurs; kCkNone when it does not; kCkNoComp when a cell of x
//   has no pair in the map.  The walk may end as soon as the range is empty -- unless the image holds a symbol without a pair
//   (`rest`): then the forward steps go on to cell k - 1, since a cell behind the one that emptied the range may be one.
//   The complement table: at most kCkMaxTable (code, comp) entries in ascending code, one per symbol of the image that the map
//   names; comp = kCkAbsent when the image does not hold the complement's value (the k-mer has a reverse complement, which
//   cannot occur).  The ticket kernel copies it to LDS and hands step() that copy; the generic form reads it from memory.
//   Bounds: q < n stays below n (KmerStepFn's argument); fm_step is in bounds on any image and returns ends in [0, n]; a
//   non-empty final [a, b) has a < n, and cnt(a) is asked only where a is a set bit of H, which is one of B.  On an image that is
//   not the BWT of a collection a final range that is no whole interval of a head counts as absent.
//   Loops: at most min(k, n) steps per item, each one forward step and at most one fm_step; the table's search halves at most
//   9 times.  One writer per entry; the only atomics are the three step counters', striped over kCkStripes slots.
static constexpr idx_t kCkNone = (idx_t)~(idx_t)0, kCkNoComp = (idx_t)(kCkNone - 1);       // (both above every row: n < 2^32 - 256 with 32-bit positions)
static constexpr u32 kCkAbsent = 0xFFFFFFFFu;
static constexpr u32 kCkMaxTable = 256;
static constexpr u64 kCkStripes = 1024;
struct CkPair { u32 code, comp; };
struct CkCodeFn {            // the i-th value of the pairs -> its symbol code, kCkAbsent when no run of the image holds it
    FmCountFn f; const u64 *vals; u32 *codes;
    GRL_DEV void operator()(u64 i) const {
        u32 c = 0, out = kCkAbsent;
        if (f.code(vals[i], c) && c != kCkAbsent) {
            u64 a = 0, b = f.R;
            for (int it = 0; it < 64 && a < b; it++) { const u64 mid = (a + b) >> 1; if (f.key[mid].below(c, 0)) a = mid + 1; else b = mid; }
            if (a < f.R && f.key[a].sym() == c) out = c;
        }
        codes[i] = out;
    }
};
struct KmerMateFn {
    typedef FmKey Key;
    typedef CkPair Pair;
    static constexpr u32 kMaxTable = kCkMaxTable;
    struct State { u64 q, a, b, t; u32 bwd, flag; };          // flag 1: the range is empty; 2: a cell without complement
    const RankCell *frc; const FmKey *key; const idx_t *slf; u64 R, n, kw;      // (kw = min(k, n) steps)
    const u64 *H; KmerCountFn cnt; const CkPair *tab; u32 nt; bool rest;
    idx_t *mate; u64 *ctr;
    GRL_HD const FmKey *keys() const { return key; }
    GRL_HD u64 n_keys() const { return R; }
    GRL_HD const CkPair *table() const { return tab; }
    GRL_HD u32 n_table() const { return nt; }
    GRL_DEV bool begin(u64 p, State &st) const {
        st.q = p; st.a = 0; st.b = n; st.t = 0; st.bwd = 0; st.flag = 0;
        return p < n && kw > 0;
    }
    // 0: c has no pair; 1: its complement is not in the image; 2: cc is the complement's code
    GRL_DEV static int comp(const CkPair *tb, u32 nt, u32 c, u32 &cc) {
        u32 a = 0, b = nt;
        for (int it = 0; it < 9 && a < b; it++) { const u32 mid = (a + b) >> 1; if (tb[mid].code < c) a = mid + 1; else b = mid; }
        if (a >= nt || tb[a].code != c) return 0;
        cc = tb[a].comp;
        return cc == kCkAbsent ? 1 : 2;
    }
    template <class TOP>
    GRL_DEV bool step(State &st, const TOP &top, const CkPair *tb) const {       // ONE forward step and at most ONE fm_step
        const u64 j = run_of_row(frc, st.q);
        const FmKey kj = key[j];
        st.q = kj.start() + (st.q - (u64)slf[j]);
        st.t++;
        u32 cc = 0;
        const int r = comp(tb, nt, kj.sym(), cc);
        if (r == 0) { st.flag = 3; return true; }
        if (!(st.flag & 1u)) {
            if (r == 1) st.flag = 1;
            else {
                u64 a = st.a, b = st.b;
                fm_step(key, slf, R, top, cc, a, b);
                st.bwd++;
                if (a >= b) st.flag = 1; else { st.a = a; st.b = b; }
            }
        }
        return st.t >= kw || ((st.flag & 1u) && !rest);
    }
    GRL_DEV void end(u64 e, const State &st) const {
        idx_t m = kCkNone;
        if (st.flag & 2u) m = kCkNoComp;
        else if (!(st.flag & 1u) && st.a < st.b && st.b <= n && lcp_bit(H, st.a) && st.b - st.a == cnt(st.a)) m = (idx_t)st.a;
        mate[e] = m;
        u64 *c = ctr + (e & (kCkStripes - 1)) * 4;
        if (st.bwd) prim::atomic_add(&c[0], (u64)st.bwd); else prim::atomic_add(&c[2], (u64)1);      // (c[2]: the heads that started no search)
        prim::atomic_add(&c[1], st.t);
    }
};
struct KmerMateEachFn {      // the generic form, prim::for_each_set_bit over H: one lane per head, the table in memory, no top level
    KmerMateFn f;
    GRL_DEV void operator()(u64 p, u64 e) const {
        KmerMateFn::State st;
        if (!f.begin(p, st)) return;
        while (!f.step(st, FmNoTop{}, f.tab)) {}
        f.end(e, st);
    }
};
struct CkRank {              // the rank of head p among the heads
    const u64 *H; const idx_t *hrank;
    GRL_DEV u64 operator()(u64 p) const { return (u64)hrank[p >> 6] + (u64)__builtin_popcountll(H[p >> 6] & ((1ull << (p & 63)) - 1ull)); }
};
struct CkRepPred {           // the representatives: the heads without a mate, or with one at or behind them
    CkRank rk; const idx_t *mate;
    GRL_DEV bool operator()(u64 p) const { return lcp_bit(rk.H, p) && (u64)mate[rk(p)] >= p; }
};
struct CkTotalFn {           // total(p) of a head p: its own rows and its mate's
    KmerCountFn cnt; CkRank rk; const idx_t *mate;
    GRL_DEV u64 operator()(u64 p) const {
        const idx_t m = mate[rk(p)];
        u64 c = cnt(p);
        if (m < kCkNoComp && (u64)m != p) c += cnt((u64)m);
        return c;
    }
};
struct CkSelPred {
    const u64 *rep; CkTotalFn tot; KmerFilter flt;
    GRL_DEV bool operator()(u64 p) const { return lcp_bit(rep, p) && flt(p, tot(p)); }
};
struct CkClassIn {           // 1 at a head that is the first of a pair (what 0), a palindrome (1), without reverse complement (2)
    CkRank rk; const idx_t *mate; int what;
    GRL_DEV u64 operator()(u64 p) const {
        if (!lcp_bit(rk.H, p)) return 0ull;
        const idx_t m = mate[rk(p)];
        if (what == 2) return m == kCkNoComp ? 1ull : 0ull;
        if (m >= kCkNoComp) return 0ull;
        return (what == 0 ? (u64)m > p : (u64)m == p) ? 1ull : 0ull;
    }
};
struct CkWindowsIn {         // KmerWindowsIn over the representatives, by total
    const u64 *rep; CkTotalFn tot;
    GRL_DEV u64 operator()(u64 p) const { return lcp_bit(rep, p) ? tot(p) : 0ull; }
};
struct CkSpectrumFn {        // KmerSpectrumFn over the representatives, by total
    CkTotalFn tot; u64 *bins; u64 last;
    GRL_DEV void operator()(u64 p, u64) const { const u64 c = tot(p); prim::atomic_add(&bins[c < last ? c : last], (u64)1); }
};
struct CkEmitFn {            // prim::for_each_set_bit over the selection: the two columns that prim::kmer_decode does not write
    CkTotalFn tot; u64 *mate_lo, *total;
    GRL_DEV void operator()(u64 p, u64 e) const {
        if (mate_lo) { const idx_t m = tot.mate[tot.rk(p)]; mate_lo[e] = m >= kCkNoComp ? ~0ull : (u64)m; }
        if (total) total[e] = tot(p);
    }
};

// ---- the compacted de Bruijn graph (grlbwt_debruijn_*).  The nodes are the selected k-mers in ascending lo; node
// v holds rows [lo, lo + count).  An in-edge of v is a symbol a above the separator that occurs in BWT[lo, lo + count): one
// backward step gives the rows [lo2, hi2) of the window a.v, which lie inside the interval of its first k cells; that interval's
// head is the last bit of B at or before lo2 (DbPrevBit, KmerCountFn's lookup in the other direction: the row's own word or the
// non-empty word in front of it, no scan over the gap), and the edge exists when the head is selected.
//   The symbols are enumerated through FmApproxFn's lower bound (the smallest symbol of the image above c), in ascending order,
//   which is ascending `from`; the enumeration ends as soon as the steps made account for all of the node's rows (the separator's
//   step first), so a node whose rows all hold one symbol stops at that symbol.
//   Loops: at most sigma symbols per node, each one lower bound and one fm_step.  Bounds: p = prev(lo2) <= lo2 < n; an entry is
//   stored only below inoff[v + 1].
static constexpr idx_t kDbNone = (idx_t)~(idx_t)0;
struct DbNodeFn {            // prim::for_each_set_bit over the selection: node e heads row p
    KmerCountFn cnt; idx_t *lo, *count;
    GRL_DEV void operator()(u64 p, u64 e) const { lo[e] = (idx_t)p; count[e] = (idx_t)cnt(p); }
};
struct DbPrevBit {           // the last bit of B at or before row q < n, or ~0
    const u64 *B; const u64 *NZ; const idx_t *nzbase; const idx_t *nzlist;
    GRL_DEV u64 operator()(u64 q) const {
        const u64 w = q >> 6;
        const u64 m = B[w] & (~0ull >> (63 - (q & 63)));
        u64 p = ~0ull;
        if (m) {
            p = w * 64 + 63 - (u64)__builtin_clzll(m);
        } else {
            const u64 r = (u64)nzbase[w >> 6] + (u64)__builtin_popcountll(NZ[w >> 6] & ((1ull << (w & 63)) - 1ull));      // non-empty words in front of w
            if (r) { const u64 x = (u64)nzlist[r - 1]; p = x * 64 + 63 - (u64)__builtin_clzll(B[x]); }
        }
        return p;
    }
};
struct DbGlobalSink {        // entry j of the edge table, stored where it belongs
    idx_t *from, *weight, *row;
    GRL_DEV void operator()(u64 j, u64 u, u64 wt, u64 r) const { from[j] = (idx_t)u; weight[j] = (idx_t)wt; row[j] = (idx_t)r; }
};
struct DbEdgeFn {
    typedef FmKey Key;
    const FmKey *key; const idx_t *slf; u64 R; u32 sep;
    DbPrevBit prev; const u64 *sel; const idx_t *selrank;
    const idx_t *nlo, *ncount;
    u32 *indeg, *outdeg; idx_t *nsteps;       // the counting pass (inoff null)
    const idx_t *inoff; u32 *bad;             // the emit pass
    GRL_HD const FmKey *keys() const { return key; }
    GRL_HD u64 n_keys() const { return R; }
    template <class TOP>
    GRL_DEV bool next_sym(u32 c, const TOP &top, u32 &out) const {      // FmApproxFn::next_sym
        if (c == ~0u) return false;
        u64 a = 0, b = R;
        top.narrow(c + 1, 0, a, b);
        for (int it = 0; it < 64 && a < b; it++) { const u64 mid = (a + b) >> 1; if (key[mid].below(c + 1, 0)) a = mid + 1; else b = mid; }
        if (a >= R) return false;
        out = key[a].sym();
        return true;
    }
    template <class TOP, class SINK>
    GRL_DEV void run(u64 v, const TOP &top, const SINK &sink) const {
        const u64 lo = (u64)nlo[v], hi = lo + (u64)ncount[v];
        const u64 base = inoff ? (u64)inoff[v] : 0, room = inoff ? (u64)inoff[v + 1] - base : 0;
        u64 a = lo, b = hi, rem = hi - lo, found = 0, steps = 1;
        fm_step(key, slf, R, top, sep, a, b);                 // the rows whose window starts its string
        rem -= b > a ? (b - a < rem ? b - a : rem) : 0;
        u32 c = sep;
        while (rem && next_sym(c, top, c)) {                  // (c goes up: at most sigma rounds)
            a = lo; b = hi;
            fm_step(key, slf, R, top, c, a, b);
            steps++;
            if (a >= b) continue;
            rem -= b - a < rem ? b - a : rem;
            const u64 p = prev(a);
            if (p == ~0ull || !lcp_bit(sel, p)) continue;
            const u64 u = rank1(sel, selrank, p);
            if (inoff) { if (found < room) sink(base + found, u, b - a, a); }
            else prim::atomic_add(&outdeg[u], 1u);
            found++;
        }
        if (inoff) { if (found != room) prim::atomic_max(bad, 1u); }
        else { indeg[v] = (u32)found; nsteps[v] = (idx_t)steps; }
    }
    template <class TOP>
    GRL_DEV void operator()(u64 v, const TOP &top) const { run(v, top, DbGlobalSink{nullptr, nullptr, nullptr}); }
};
struct DbEdgeLaneFn {        // the emit pass: one lane per node that stores its own entries
    typedef FmKey Key;
    DbEdgeFn f; DbGlobalSink sink;
    GRL_HD const FmKey *keys() const { return f.key; }
    GRL_HD u64 n_keys() const { return f.R; }
    template <class TOP>
    GRL_DEV void operator()(u64 v, const TOP &top) const { f.run(v, top, sink); }
    GRL_DEV void operator()(u64 v) const { f.run(v, FmNoTop{}, sink); }
};
struct DbDegIn {
    const u32 *d;
    GRL_DEV u64 operator()(u64 v) const { return (u64)d[v]; }
};
// The unitigs.  link[v] = the node in front of v on its unitig, none where v heads one: v's only in-edge u -> v with
// out_degree[u] = 1.  u then has no other out-edge, so link is one-to-one and succ[u] = v has one writer.  mark[v]: 0 inside a
// unitig, 1 a head, 2 the head of a circular one (a self-loop links a node to itself, so "head" cannot be "points at itself").
//   Pointer jumping: (ptr, dist, mn) of v says that ptr lies dist links in front of v and mn is the smallest id among the dist
//   nodes from v on; a round doubles dist unless v or ptr is a head.  After r rounds every node within 2^r links of a head has
//   found it, and a node on a cycle has seen min(2^r, the cycle) of its nodes: after ceil(log2 n_nodes) + 1 rounds its mn is the
//   cycle's smallest id.  That node becomes the head (mark 2), and the same rounds rank the cycle's nodes behind it.
struct DbLinkFn {
    const u32 *indeg, *outdeg; const idx_t *inoff, *from; idx_t *link, *succ;
    GRL_DEV void operator()(u64 v) const {
        idx_t l = kDbNone;
        if (indeg[v] == 1u) {
            const idx_t u = from[(u64)inoff[v]];
            if (outdeg[(u64)u] == 1u) { l = u; succ[(u64)u] = (idx_t)v; }
        }
        link[v] = l;
    }
};
struct DbJumpInitFn {        // open: only the nodes that found no head are set up again (the second set of rounds; null: all)
    const idx_t *link; const u8 *mark; const u8 *open; idx_t *ptr, *dist, *mn;
    GRL_DEV void operator()(u64 v) const {
        if (open && !open[v]) return;
        const bool head = mark[v] != 0;
        ptr[v] = head ? (idx_t)v : link[v]; dist[v] = head ? (idx_t)0 : (idx_t)1; mn[v] = (idx_t)v;
    }
};
struct DbMarkFn {
    const idx_t *link; u8 *mark;
    GRL_DEV void operator()(u64 v) const { mark[v] = link[v] == kDbNone ? 1 : 0; }
};
struct DbJumpFn {            // one round, from generation 0 to generation 1
    const u8 *mark; const idx_t *p0, *d0, *m0; idx_t *p1, *d1, *m1;
    GRL_DEV void operator()(u64 v) const {
        const idx_t p = p0[v];
        idx_t q = p, d = d0[v], m = m0[v];
        if (!mark[v] && !mark[(u64)p]) {
            q = p0[(u64)p]; d = (idx_t)(d + d0[(u64)p]);
            const idx_t o = m0[(u64)p];
            m = o < m ? o : m;
        }
        p1[v] = q; d1[v] = d; m1[v] = m;
    }
};
struct DbOpenIn {            // 1 for a node that has found no head yet
    const u8 *mark; const idx_t *ptr;
    GRL_DEV u64 operator()(u64 v) const { return !mark[v] && !mark[(u64)ptr[v]] ? 1ull : 0ull; }
};
struct DbCycleHeadFn {       // the smallest node of every cycle becomes its head; `open` is read, mark written: two arrays
    const u8 *open; const idx_t *mn; u8 *mark;
    GRL_DEV void operator()(u64 v) const { if (open[v] && (u64)mn[v] == v) mark[v] = 2; }
};
struct DbOpenFn {
    const u8 *mark; const idx_t *ptr; u8 *open;
    GRL_DEV void operator()(u64 v) const { open[v] = !mark[v] && !mark[(u64)ptr[v]] ? 1 : 0; }
};
struct DbMarkIn {
    const u8 *mark; u8 what;     // 0: any head
    GRL_DEV u64 operator()(u64 v) const { return (what ? mark[v] == what : mark[v] != 0) ? 1ull : 0ull; }
};
struct DbPlaceFn {           // unitig and rank of every node; the tails give the lengths (one tail per unitig)
    const u8 *mark; const idx_t *ptr, *dist, *hrank, *succ; idx_t *unitig, *rank, *ulen; u8 *ucirc;
    GRL_DEV void operator()(u64 v) const {
        const u64 h = (u64)ptr[v], j = (u64)hrank[h];
        unitig[v] = (idx_t)j; rank[v] = dist[v];
        const idx_t s = succ[v];
        if (s == kDbNone || mark[(u64)s]) ulen[j] = (idx_t)(dist[v] + 1);
        if (mark[v]) ucirc[j] = mark[v] == 2 ? 1 : 0;
    }
};
struct DbOrderFn {
    const idx_t *unitig, *rank, *uoff; idx_t *nodes;
    GRL_DEV void operator()(u64 v) const { nodes[(u64)uoff[(u64)unitig[v]] + (u64)rank[v]] = (idx_t)v; }
};
struct DbCountOfIn {         // the count of the i-th node in unitig order
    const idx_t *nodes, *count;
    GRL_DEV u64 operator()(u64 i) const { return (u64)count[(u64)nodes[i]]; }
};
struct DbWeightFn {
    const idx_t *uoff; const u64 *wsum; idx_t *uweight;
    GRL_DEV void operator()(u64 j) const { uweight[j] = (idx_t)(wsum[(u64)uoff[j + 1]] - wsum[(u64)uoff[j]]); }
};
template <class S, class D>
struct DbCopyFn {            // the writers: the handle's arrays in the widths of the interface
    const S *src; D *dst;
    GRL_DEV void operator()(u64 i) const { dst[i] = (D)src[i]; }
};
// The cells.  Unitig j of m nodes takes cells [off[j] + j (k - 1), off[j + 1] + (j + 1)(k - 1)): place r < m holds the first cell
// of its r-th node -- the symbol of the sorted run that holds the node's row lo, no walk -- and the k - 1 cells behind them are
// the forward steps from the last node's lo (KmerStepFn; the first step gives that node's own first cell again).
//   Bounds: lo < n, so run_of_row answers a run below R; a cell index is below n_nodes + n_unitigs (k - 1).
template <class cell_t>
struct DbFirstCellFn {       // for_each over the nodes in unitig order
    KmerStepFn step; const idx_t *nodes, *unitig, *nlo; u64 k; cell_t *cells;
    GRL_DEV void operator()(u64 i) const {
        const u64 v = (u64)nodes[i];
        u64 q = (u64)nlo[v];
        cells[i + (u64)unitig[v] * (k - 1)] = (cell_t)step(q);
    }
};
template <class cell_t>
struct DbTailCellsFn {       // for_each over the unitigs: k - 1 dependent steps each
    KmerStepFn step; const idx_t *nodes, *uoff, *nlo; u64 k; cell_t *cells;
    GRL_DEV void operator()(u64 j) const {
        const u64 e = (u64)uoff[j + 1];
        u64 q = (u64)nlo[(u64)nodes[e - 1]];
        (void)step(q);
        cell_t *out = cells + e + j * (k - 1);
        for (u64 t = 0; t + 1 < k; t++) out[t] = (cell_t)step(q);
    }
};
struct DbPrintIn {           // the index's fingerprint: a sum over the sorted runs
    const FmKey *key; const idx_t *slf;
    GRL_DEV u64 operator()(u64 j) const {
        const FmKey kj = key[j];
        return ((u64)kj.sym() * 0x9E3779B97F4A7C15ull + kj.start() * 0xC2B2AE3D27D4EB4Full + (u64)slf[j]) * (2 * j + 1);
    }
};

// ---- the strand-merged compacted de Bruijn graph (grlbwt_cdebruijn_*).  Node v is the v-th selected class of
// grlbwt_fm_kmers_canonical: its representative's rows [lo, lo + count), its mate's head (kCkNone, kCkNoComp as there) and
// its total.  End 2 v is in front of the representative's first cell, end 2 v + 1 behind its last; a palindrome has end 0 only.
//   The edge search is 4n's, run from every head -- representative or mate -- whose class is selected: a symbol a in front of
//   head s gives the window w = a.s, whose first k cells are headed by p = prev(lo(w)).  w leaves p's node through end 1 when p
//   is the representative and 0 when it is the mate (or a palindrome), and enters s's node through end 0 when s is the
//   representative and 1 when it is the mate.  Each such w is one FORWARD record (source end, other end, lo(w), occ(w)); record
//   nf + r is the REVERSE of forward record r (other end, source end, weight only), void when the two ends are one (a hairpin).
//   Two stable sorts of the record numbers, by other end and then by source end, put the records of one (source, other) side
//   by side: w's forward record and the reverse record of rc(w), never more than two and never two forward ones.
//   Loops: at most sigma symbols per head and pass; the merge looks at two neighbours; a lower bound halves at most 64 times.
//   Bounds: a head's records are stored only below roff[i + 1]; an entry only below the number of group heads; end ids are
//   below 2 n_nodes, the sentinel 2 n_nodes is the key of the void records alone.  Nothing waits for another thread.
struct CdbHeadOf {           // head p -> its node, whether p is the class's mate, whether it is a palindrome
    const u64 *H; CkRank rk; const idx_t *mate; const u64 *sel; const idx_t *selrank;
    GRL_DEV bool operator()(u64 p, u64 &node, u32 &is_mate, u32 &pal) const {
        if (!lcp_bit(H, p)) return false;
        const idx_t m = mate[rk(p)];
        const u64 r = (m < kCkNoComp && (u64)m < p) ? (u64)m : p;
        if (!lcp_bit(sel, r)) return false;
        node = rank1(sel, selrank, r); is_mate = r != p ? 1u : 0u; pal = (m < kCkNoComp && (u64)m == p) ? 1u : 0u;
        return true;
    }
};
struct CdbHeadPred {         // the heads whose class is selected
    CdbHeadOf h;
    GRL_DEV bool operator()(u64 p) const { u64 v; u32 a, b; return h(p, v, a, b); }
};
struct CdbNodeFn {           // prim::for_each_set_bit over the selection: node e is the class of representative p
    CkTotalFn tot; idx_t *lo, *count, *mate, *total;
    GRL_DEV void operator()(u64 p, u64 e) const { lo[e] = (idx_t)p; count[e] = (idx_t)tot.cnt(p); mate[e] = tot.mate[tot.rk(p)]; total[e] = (idx_t)tot(p); }
};
struct CdbHeadListFn {       // prim::for_each_set_bit over the selected heads: rows, and the end the head's k-mer is entered through
    CdbHeadOf h; KmerCountFn cnt; idx_t *hlo, *hcount, *hend;
    GRL_DEV void operator()(u64 p, u64 i) const {
        u64 v = 0; u32 m = 0, pal = 0;
        (void)h(p, v, m, pal);
        hlo[i] = (idx_t)p; hcount[i] = (idx_t)cnt(p); hend[i] = (idx_t)(2 * v + m);
    }
};
struct CdbEdgeFn {           // DbEdgeFn::run with a sink that writes records; roff null: the counting pass
    typedef FmKey Key;
    DbEdgeFn e;              // (key, slf, R, sep, prev and next_sym; the rest of it is not used)
    CdbHeadOf head;
    const idx_t *hlo, *hcount, *hend;
    idx_t *found_of, *nsteps;
    const idx_t *roff; idx_t *rsrc, *roth, *rlo, *rocc; u32 *bad;
    GRL_HD const FmKey *keys() const { return e.key; }
    GRL_HD u64 n_keys() const { return e.R; }
    template <class TOP>
    GRL_DEV void operator()(u64 i, const TOP &top) const {
        const u64 lo = (u64)hlo[i], hi = lo + (u64)hcount[i];
        const u64 base = roff ? (u64)roff[i] : 0, room = roff ? (u64)roff[i + 1] - base : 0;
        u64 a = lo, b = hi, rem = hi - lo, found = 0, steps = 1;
        fm_step(e.key, e.slf, e.R, top, e.sep, a, b);         // the rows whose window starts its string
        rem -= b > a ? (b - a < rem ? b - a : rem) : 0;
        u32 c = e.sep;
        while (rem && e.next_sym(c, top, c)) {                // (c goes up: at most sigma rounds)
            a = lo; b = hi;
            fm_step(e.key, e.slf, e.R, top, c, a, b);
            steps++;
            if (a >= b) continue;
            rem -= b - a < rem ? b - a : rem;
            const u64 p = e.prev(a);
            u64 u = 0; u32 um = 0, upal = 0;
            if (p == ~0ull || !head(p, u, um, upal)) continue;
            if (roff && found < room) {
                const u64 j = base + found;
                rsrc[j] = (idx_t)(2 * u + ((um | upal) ? 0u : 1u)); roth[j] = hend[i]; rlo[j] = (idx_t)a; rocc[j] = (idx_t)(b - a);
            }
            found++;
        }
        if (roff) { if (found != room) prim::atomic_max(bad, 1u); }
        else { found_of[i] = (idx_t)found; nsteps[i] = (idx_t)steps; }
    }
    GRL_DEV void operator()(u64 i) const { (*this)(i, FmNoTop{}); }
};
struct CdbRec {              // record r of 2 nf; `none` = 2 n_nodes keys the void records
    const idx_t *src, *oth; u64 nf, none;
    GRL_DEV u64 source(u64 r) const { if (r < nf) return (u64)src[r]; r -= nf; return src[r] == oth[r] ? none : (u64)oth[r]; }
    GRL_DEV u64 other(u64 r) const { if (r < nf) return (u64)oth[r]; r -= nf; return src[r] == oth[r] ? none : (u64)src[r]; }
};
struct CdbKeyFn {            // the sort keys: pass 0 the other end of record i, pass 1 the source end of the record at place i
    CdbRec rec; const idx_t *perm; idx_t *key, *val;
    GRL_DEV void operator()(u64 i) const {
        if (perm) key[i] = (idx_t)rec.source((u64)perm[i]);
        else { key[i] = (idx_t)rec.other(i); val[i] = (idx_t)i; }
    }
};
struct CdbGroupHeadIn {      // 1 at the first record of every (source, other) in sorted order; the void records are none
    CdbRec rec; const idx_t *perm;
    GRL_DEV u64 operator()(u64 i) const {
        const u64 r = (u64)perm[i], s = rec.source(r);
        if (s == rec.none) return 0ull;
        if (i == 0) return 1ull;
        const u64 q = (u64)perm[i - 1];
        return rec.source(q) != s || rec.other(q) != rec.other(r) ? 1ull : 0ull;
    }
};
struct CdbHairpinIn {
    const idx_t *src, *oth;
    GRL_DEV u64 operator()(u64 r) const { return src[r] == oth[r] ? 1ull : 0ull; }
};
// the merge of one group, shared by the generic form and the tile kernel: entry j from the records at places i, i + 1
struct CdbMerge {
    CdbRec rec; const idx_t *perm, *rlo, *rocc; u64 nrec;
    idx_t *esrc, *eoth, *ew, *erow, *ecnt; u32 *bad;
    GRL_DEV void operator()(u64 i, u64 j) const {
        const u64 r = (u64)perm[i], s = rec.source(r), o = rec.other(r);
        u64 w = (u64)rocc[r < rec.nf ? r : r - rec.nf], row = (u64)kDbNone, cnt = 0;
        u32 fwd = 0;
        if (r < rec.nf) { row = (u64)rlo[r]; cnt = (u64)rocc[r]; fwd = 1; }
        if (i + 1 < nrec) {
            const u64 r2 = (u64)perm[i + 1];
            if (rec.source(r2) == s && rec.other(r2) == o) {
                w += (u64)rocc[r2 < rec.nf ? r2 : r2 - rec.nf];
                if (r2 < rec.nf) { row = (u64)rlo[r2]; cnt = (u64)rocc[r2]; fwd++; }
                if (i + 2 < nrec) { const u64 r3 = (u64)perm[i + 2]; if (rec.source(r3) == s && rec.other(r3) == o) prim::atomic_max(bad, 1u); }
            }
        }
        if (fwd > 1) prim::atomic_max(bad, 1u);
        esrc[j] = (idx_t)s; eoth[j] = (idx_t)o; ew[j] = (idx_t)w; erow[j] = (idx_t)row; ecnt[j] = (idx_t)cnt;
    }
};
struct CdbMergeEachFn {      // the generic form of the merge: for_each over the sorted records
    CdbGroupHeadIn head; const idx_t *eidx; CdbMerge merge;
    GRL_DEV void operator()(u64 i) const { if (head(i)) merge(i, (u64)eidx[i]); }
};
struct CdbEndOffFn {         // end_offsets[a] = the entries whose source end is below a: a lower bound in the entries' sources
    const idx_t *esrc; u64 nhe; idx_t *endoff;
    GRL_DEV void operator()(u64 a) const {
        u64 x = 0, y = nhe;
        for (int it = 0; it < 64 && x < y; it++) { const u64 mid = (x + y) >> 1; if ((u64)esrc[mid] < a) x = mid + 1; else y = mid; }
        endoff[a] = (idx_t)x;
    }
};
struct CdbEndDegIn {
    const idx_t *endoff;
    GRL_DEV u64 operator()(u64 a) const { return (u64)endoff[a + 1] - (u64)endoff[a]; }
};
struct CdbSelfIn {           // the entries whose other end is their source end: the hairpins
    const idx_t *esrc, *eoth;
    GRL_DEV u64 operator()(u64 j) const { return esrc[j] == eoth[j] ? 1ull : 0ull; }
};
struct CdbNodeKindIn {       // what 0: rigid nodes; 1: palindromes; 2: nodes whose reverse complement does not occur
    const idx_t *nlo, *nmate; int what;
    GRL_DEV u64 operator()(u64 v) const {
        const idx_t m = nmate[v];
        if (what == 2) return m == kCkNone ? 1ull : 0ull;
        const bool pal = m == nlo[v];
        return (what == 1 ? pal : (pal || m == kCkNoComp)) ? 1ull : 0ull;
    }
};
// The unitigs, on the doubled graph of the 2 n_nodes oriented nodes x = 2 v + o (o = 1: v read as the reverse complement of its
// representative).  Reading (v, o) leaves v through end 1 - o, which is end id x ^ 1, and was entered through end o, id x.  An
// end's partner is the other end of its only half-edge when that half-edge is compactable -- both ends of degree 1, two
// different ends, neither node rigid, and the partner's half-edge leads back (it does on the BWT of a collection; the test keeps
// succ and link inverse to each other on any image).  succ(x) = partner(x ^ 1), link(x) = partner(x) ^ 1.  x -> x ^ 1 maps a
// chain onto its reverse; a chain that held both x and x ^ 1 would be mapped onto itself, with a fixed node (impossible) or a
// fixed link, partner(a) = a, which is excluded: every unitig appears as two disjoint chains, and 4n's rounds run as they are.
struct CdbEnds {
    const idx_t *endoff, *eoth, *nlo, *nmate;
    GRL_DEV bool rigid(u64 v) const { const idx_t m = nmate[v]; return m == kCkNoComp || m == nlo[v]; }
    GRL_DEV u64 deg(u64 a) const { return (u64)endoff[a + 1] - (u64)endoff[a]; }
    GRL_DEV u64 partner(u64 a) const {
        if (deg(a) != 1) return ~0ull;
        const u64 b = (u64)eoth[(u64)endoff[a]];
        if (b == a || deg(b) != 1 || (u64)eoth[(u64)endoff[b]] != a || rigid(a >> 1) || rigid(b >> 1)) return ~0ull;
        return b;
    }
};
struct CdbLinkFn {
    CdbEnds E; idx_t *link, *succ;
    GRL_DEV void operator()(u64 x) const {
        const u64 b = E.partner(x), s = E.partner(x ^ 1);
        link[x] = b == ~0ull ? kDbNone : (idx_t)(b ^ 1);
        succ[x] = s == ~0ull ? kDbNone : (idx_t)s;
    }
};
// Which of a unitig's two chains is reported, decided at the chain's tail, which knows its head after the rounds: a path keeps
// the chain whose head node has the smaller id of the two end nodes (the other chain's head is this tail reversed), a single
// node its + reading, a cycle the chain whose head -- its smallest oriented id -- is even.  One tail per chain: one writer.
struct CdbKeepFn {
    const u8 *mark; const idx_t *ptr, *succ; u8 *keep;
    GRL_DEV void operator()(u64 x) const {
        const idx_t s = succ[x];
        if (s != kDbNone && !mark[(u64)s]) return;
        const u64 h = (u64)ptr[x];
        keep[h] = (mark[h] == 2 ? !(h & 1) : ((h >> 1) < (x >> 1) || (h == x && !(x & 1)))) ? 1 : 0;
    }
};
struct CdbKeptIn {           // 1 at the head of a reported chain (what 2: of a circular one)
    const u8 *mark, *keep; u8 what;
    GRL_DEV u64 operator()(u64 x) const { return (what ? mark[x] == what : mark[x] != 0) && keep[x] ? 1ull : 0ull; }
};
struct CdbPlaceFn {
    const u8 *mark, *keep; const idx_t *ptr, *dist, *hrank, *succ; idx_t *unitig, *rank, *ulen; u8 *orient, *ucirc;
    GRL_DEV void operator()(u64 x) const {
        const u64 h = (u64)ptr[x];
        if (!keep[h]) return;
        const u64 j = (u64)hrank[h], v = x >> 1;
        unitig[v] = (idx_t)j; rank[v] = dist[x]; orient[v] = (u8)(x & 1);
        const idx_t s = succ[x];
        if (s == kDbNone || mark[(u64)s]) ulen[j] = (idx_t)(dist[x] + 1);
        if (mark[x]) ucirc[j] = mark[x] == 2 ? 1 : 0;
    }
};
struct CdbOrderFn {          // the oriented nodes in unitig order
    const idx_t *unitig, *rank, *uoff; const u8 *orient; idx_t *nodes;
    GRL_DEV void operator()(u64 v) const { nodes[(u64)uoff[(u64)unitig[v]] + (u64)rank[v]] = (idx_t)(2 * v + orient[v]); }
};
struct CdbTotalOfIn {
    const idx_t *nodes, *total;
    GRL_DEV u64 operator()(u64 i) const { return (u64)total[(u64)nodes[i] >> 1]; }
};
struct CdbCopyRowFn {        // fwd_row: the handle's "none" in the interface's width
    const idx_t *src; u64 *dst;
    GRL_DEV void operator()(u64 i) const { dst[i] = src[i] == kDbNone ? ~0ull : (u64)src[i]; }
};
struct CdbDegreeFn {
    const idx_t *endoff; u32 *d0, *d1;
    GRL_DEV void operator()(u64 v) const {
        if (d0) d0[v] = (u32)((u64)endoff[2 * v + 1] - (u64)endoff[2 * v]);
        if (d1) d1[v] = (u32)((u64)endoff[2 * v + 2] - (u64)endoff[2 * v + 1]);
    }
};
// The cells.  Place r < m of a unitig holds the first cell of its r-th oriented node (v, o): o = 0, the symbol of the sorted run
// that holds lo; o = 1 with a mate, the same at mate_lo; o = 1 without one, the complement of the representative's LAST cell, k
// forward steps from lo (a "walk").  The k - 1 cells behind come from the last oriented node: forward steps from lo or mate_lo,
// or, without a mate, the complements of the representative's first k - 1 cells in reverse.  The complement is taken on symbol
// codes through the handle's table (code -> the complement's VALUE, which the image need not hold).
//   Bounds: KmerStepFn's (rows stay below n); a cell index is below n_nodes + n_unitigs (k - 1).
struct CdbStepFn {
    KmerStepFn s; const u32 *ccode; const u64 *cval; u32 nt;
    GRL_DEV u32 code(u64 &q) const {
        const u64 j = run_of_row(s.frc, q);
        const FmKey kj = s.key[j];
        q = kj.start() + (q - (u64)s.slf[j]);
        return kj.sym();
    }
    GRL_DEV u64 val(u32 c) const { return s.alpha ? s.alpha[c] : (u64)c; }
    GRL_DEV u64 comp(const u32 *cc, u32 c) const {      // cc: the codes, in memory or in LDS
        u32 a = 0, b = nt;
        for (int it = 0; it < 9 && a < b; it++) { const u32 mid = (a + b) >> 1; if (cc[mid] < c) a = mid + 1; else b = mid; }
        return a < nt && cc[a] == c ? cval[a] : 0ull;
    }
};
struct CdbCellSrc {          // where the first cell of oriented node x comes from: a row (walk false) or a walk from a row
    const idx_t *nlo, *nmate;
    GRL_DEV u64 operator()(u64 x, bool &walk) const {
        const u64 v = x >> 1;
        walk = false;
        if (!(x & 1)) return (u64)nlo[v];
        const idx_t m = nmate[v];
        if (m < kCkNoComp) return (u64)m;
        walk = true;
        return (u64)nlo[v];
    }
};
template <class cell_t>
struct CdbFirstCellFn {      // the generic form, for_each over the nodes in unitig order; the walks inline
    CdbStepFn st; CdbCellSrc src; const idx_t *nodes, *unitig; u64 k; cell_t *cells;
    GRL_DEV void operator()(u64 i) const {
        const u64 x = (u64)nodes[i];
        bool walk;
        u64 q = src(x, walk);
        u32 c = st.code(q);
        if (walk) for (u64 t = 1; t < k; t++) c = st.code(q);
        cells[i + (u64)unitig[x >> 1] * (k - 1)] = (cell_t)(walk ? st.comp(st.ccode, c) : st.val(c));
    }
};
struct CdbWalkPred {         // the places in unitig order that take a walk
    CdbCellSrc src; const idx_t *nodes;
    GRL_DEV bool operator()(u64 i) const { bool walk; (void)src((u64)nodes[i], walk); return walk; }
};
struct CdbWalkIn {
    CdbWalkPred p;
    GRL_DEV u64 operator()(u64 i) const { return p(i) ? 1ull : 0ull; }
};
struct CdbCopyMateFn {       // mate_lo as grlbwt_fm_kmers_canonical writes it
    const idx_t *src; u64 *dst;
    GRL_DEV void operator()(u64 v) const { dst[v] = src[v] >= kCkNoComp ? ~0ull : (u64)src[v]; }
};
struct CdbWalkListFn {
    idx_t *list;
    GRL_DEV void operator()(u64 i, u64 t) const { list[t] = (idx_t)i; }
};
template <class cell_t>
struct CdbWalkFn {           // prim::walk_tickets: ticket t is the t-th place that takes a walk
    struct State { u64 q, left; u32 c; };
    CdbStepFn st; const idx_t *list, *nodes, *nlo, *unitig; u64 k; cell_t *cells;
    GRL_DEV bool begin(u64 t, State &s) const { s.q = (u64)nlo[(u64)nodes[(u64)list[t]] >> 1]; s.left = k; s.c = 0; return k > 0; }
    GRL_DEV bool step(State &s) const { s.c = st.code(s.q); return --s.left == 0; }
    GRL_DEV void end(u64 t, const State &s) const {
        const u64 i = (u64)list[t];
        cells[i + (u64)unitig[(u64)nodes[i] >> 1] * (k - 1)] = (cell_t)st.comp(st.ccode, s.c);
    }
};
template <class cell_t>
struct CdbTailCellsFn {      // for_each over the unitigs: k - 1 dependent steps each
    CdbStepFn st; CdbCellSrc src; const idx_t *nodes, *uoff; u64 k; cell_t *cells;
    GRL_DEV void operator()(u64 j) const {
        const u64 e = (u64)uoff[j + 1];
        bool walk;
        u64 q = src((u64)nodes[e - 1], walk);
        cell_t *out = cells + e + j * (k - 1);
        if (!walk) {
            (void)st.code(q);
            for (u64 t = 0; t + 1 < k; t++) out[t] = (cell_t)st.val(st.code(q));
        } else {
            for (u64 t = 0; t + 1 < k; t++) out[k - 2 - t] = (cell_t)st.comp(st.ccode, st.code(q));
        }
    }
};

// ---- the right-maximal and maximal repeats (grlbwt_fm_repeats).  V[p] = min(LCP[p], cap) in the narrowest width
// that holds cap.  Row p with V[p] = v >= 1 is the split row of a right-maximal repeat of v cells exactly when the nearest q < p
// with V[q] <= v has V[q] < v; the repeat's rows are then [q, e), e the nearest row behind p with V[e] < v, or n.  Both are
// nearest-smaller-value searches, answered through a tree of minima: level 0 is V, an entry of level l + 1 the minimum of a
// node of kRepFanout consecutive entries of level l, up to the first level that is one node.  The levels lie back to back in
// one array, level l at rep_off(n, l) with rep_cnt(n, l) = ceil(n / 64^l) entries, so a search carries (level, index) and
// needs no table.  A search scans the entries of its own node on its side, then climbs: at each level the siblings of its
// ancestor on that side, nearest first; at the first that qualifies it descends, at each level to the nearest child that
// qualifies (the node's minimum does, so one child does).
//   Loops: the climb and the descent take at most kRepFanout reads per level each, 2 * levels * kRepFanout per search.
//   Bounds: a level's index stays below rep_cnt of that level: the backward scan goes down from an index that is, the forward
//   scan and both descents clamp at it (child i * 64 of entry i < ceil(c / 64) is below c).  Nothing waits for another thread.
static constexpr u64 kRepFanout = 64;
GRL_HD u64 rep_cnt(u64 n, u32 l) { return ((n - 1) >> (6 * l)) + 1; }               // (n >= 1, l <= 10)
static inline u32 rep_levels(u64 n) { u32 L = 1; while (rep_cnt(n, L - 1) > kRepFanout) L++; return L; }
static inline u64 rep_entries(u64 n) { u64 s = 0; for (u32 l = 0; l < rep_levels(n); l++) s += rep_cnt(n, l); return s; }
template <class VT>
struct RepGlobalRd {         // entry j of level l, which starts at `off`
    const VT *tree;
    GRL_DEV u64 operator()(u32, u64 off, u64 j) const { return (u64)tree[off + j]; }
};
static constexpr u64 kRepNone = ~0ull;
// the nearest q < p with V[q] <= v, or kRepNone; top = the highest level the search looked at
template <class RD>
GRL_DEV u64 rep_search_back(const RD &rd, u64 n, u32 levels, u64 p, u64 v, u32 &top) {
    u64 i = p, off = 0;
    u32 l = 0;
    bool found = false;
    while (l < levels) {
        const u64 base = i & ~(kRepFanout - 1);
        u64 j = i;
        while (j > base) {
            j--;
            if (rd(l, off, j) <= v) { found = true; break; }
        }
        if (found) { i = j; break; }
        off += rep_cnt(n, l);
        l++; i >>= 6;
    }
    top = l < levels ? l : levels - 1;
    if (!found) return kRepNone;
    while (l > 0) {
        l--;
        const u64 c = rep_cnt(n, l), first = i * kRepFanout;
        off -= c;
        u64 j = first + kRepFanout - 1 < c ? first + kRepFanout - 1 : c - 1;
        while (j > first && !(rd(l, off, j) <= v)) j--;
        i = j;
    }
    return i;
}
// the nearest q > p with V[q] < v, or n
template <class RD>
GRL_DEV u64 rep_search_fwd(const RD &rd, u64 n, u32 levels, u64 p, u64 v, u32 &top) {
    u64 i = p, off = 0;
    u32 l = 0;
    bool found = false;
    while (l < levels) {
        const u64 c = rep_cnt(n, l);
        const u64 end = (i | (kRepFanout - 1)) + 1 < c ? (i | (kRepFanout - 1)) + 1 : c;
        u64 j = i + 1;
        for (; j < end; j++)
            if (rd(l, off, j) < v) { found = true; break; }
        if (found) { i = j; break; }
        off += c;
        l++; i >>= 6;
    }
    top = l < levels ? l : levels - 1;
    if (!found) return n;
    while (l > 0) {
        l--;
        const u64 c = rep_cnt(n, l), first = i * kRepFanout;
        off -= c;
        const u64 end = first + kRepFanout < c ? first + kRepFanout : c;
        u64 j = first;
        while (j + 1 < end && !(rd(l, off, j) < v)) j++;
        i = j;
    }
    return i;
}
template <class VT>
struct RepMinFn {            // the generic form of a level: entry i = the minimum of its node
    const VT *src; u64 ns; VT *dst;
    GRL_DEV void operator()(u64 i) const {
        const u64 a = i * kRepFanout, b = a + kRepFanout < ns ? a + kRepFanout : ns;
        VT m = src[a];
        for (u64 j = a + 1; j < b; j++) m = src[j] < m ? src[j] : m;
        dst[i] = m;
    }
};
// Left-maximality.  HB has a bit at every row whose BWT symbol is the separator and at the first row of every record that does
// not continue the record in front of it with the same symbol (a foreign image may split a run): the rows at which the BWT
// symbol may differ from the row before.  Rows [lo, e) hold one and the same symbol that is not the separator exactly when
// HB has no bit in (lo, e): a separator at row lo is seen at row lo + 1 < e, which is a separator's row or a record's first.
// The records are read in F order, sorted by (symbol, start): a record continues its predecessor there when it continues it in the BWT.
struct RepHeadFn {           // for_each over the R records
    const FmKey *key; const idx_t *slf; u64 n; u64 *hb;
    GRL_DEV void operator()(u64 j) const {
        const FmKey kj = key[j];
        const u64 pos = kj.start();
        if ((u64)slf[j + 1] == (u64)slf[j] || pos >= n) return;            // (an empty record heads nothing)
        if (j) {
            const FmKey kp = key[j - 1];
            if (kp.sym() == kj.sym() && kp.start() + ((u64)slf[j] - (u64)slf[j - 1]) == pos) return;
        }
        prim::atomic_or(&hb[pos >> 6], 1ull << (pos & 63));
    }
};
struct RepSepFn {            // for_each over the n_strings rows of F that start with the separator: their BWT positions (KmerStepFn's step)
    const RankCell *frc; const FmKey *key; const idx_t *slf; u64 n; u64 *hb;
    GRL_DEV void operator()(u64 i) const {
        const u64 j = run_of_row(frc, i);
        const u64 pos = key[j].start() + (i - (u64)slf[j]);
        if (pos < n) prim::atomic_or(&hb[pos >> 6], 1ull << (pos & 63));
    }
};
struct RepHeads {            // is the repeat of rows [lo, e) left-maximal
    const u64 *hb; const idx_t *hrank;
    GRL_DEV bool operator()(u64 lo, u64 e) const { return rank1(hb, hrank, e) > rank1(hb, hrank, lo + 1); }
};
struct RepFilter {           // the table's entries among the repeats inside the length bounds
    u64 rb, re, cmin, cmax; bool maximal;
    GRL_DEV bool operator()(u64 p, u64 count, bool mx) const { return p >= rb && p < re && count >= cmin && count <= cmax && (mx || !maximal); }
};
struct RepRowFn {            // the repeat that row p, of value v, splits: its rows [lo, e) and whether it is left-maximal
    u64 n; u32 levels; u64 minl, maxl; RepHeads heads; RepFilter flt;
    // far: the searches of this row, 0 to 2, that looked above level 1 -- in the tile kernel, that left their tile
    template <class RD>
    GRL_DEV bool operator()(const RD &rd, u64 p, u64 v, u64 &lo, u64 &e, bool &mx, u32 &far) const {
        far = 0;
        if (v < minl || v > maxl) return false;
        u32 top = 0;
        lo = rep_search_back(rd, n, levels, p, v, top);
        far += top >= 2u ? 1u : 0u;
        if (lo == kRepNone || rd(0, 0, lo) >= v) return false;
        e = rep_search_fwd(rd, n, levels, p, v, top);
        far += top >= 2u ? 1u : 0u;
        mx = heads(lo, e);
        return true;
    }
};
template <class VT>
struct RepStatIn {           // the generic form's counters: 0 the repeats, 1 the maximal ones, 2 their lengths, 3 their counts
    const VT *tree; RepRowFn row; int f;
    GRL_DEV u64 operator()(u64 p) const {
        u64 lo = 0, e = 0;
        bool mx = false;
        u32 top;
        const u64 v = (u64)tree[p];
        if (!row(RepGlobalRd<VT>{tree}, p, v, lo, e, mx, top)) return 0;
        return f == 0 ? 1ull : f == 1 ? (mx ? 1ull : 0ull) : f == 2 ? v : e - lo;
    }
};
template <class VT>
struct RepSelPred {
    const VT *tree; RepRowFn row;
    GRL_DEV bool operator()(u64 p) const {
        u64 lo = 0, e = 0;
        bool mx = false;
        u32 top;
        return row(RepGlobalRd<VT>{tree}, p, (u64)tree[p], lo, e, mx, top) && row.flt(p, e - lo, mx);
    }
};
template <class VT>
struct RepEmitFn {           // the emit of both forms, prim::for_each_set_bit over the selected rows: the two searches once more, in the tree in memory
    const VT *tree; RepRowFn row; u64 *lo, *count, *len, *split;
    GRL_DEV void operator()(u64 p, u64 e) const {
        u64 a = 0, b = 0;
        bool mx = false;
        u32 top;
        const u64 v = (u64)tree[p];
        (void)row(RepGlobalRd<VT>{tree}, p, v, a, b, mx, top);
        if (lo) lo[e] = a;
        if (count) count[e] = b - a;
        if (len) len[e] = v;
        if (split) split[e] = p;
    }
};

struct Image {
    // ---- opening an image: the one parse of the 16 header bytes, the one test of a cell width, the one dispatch on it -------
    struct ImageHeader {
        u64 sb, fb, R;
        ImageRecs recs(const void *dev_image) const { return ImageRecs{(const u8 *)dev_image, (u32)sb, (u32)fb}; }
    };
    static ImageHeader image_header(const void *dev_image, u64 image_bytes) {
        if (image_bytes < 16) throw prim::Error(-22, "not an .rl_bwt image");
        u64 hdr[2];
        prim::d2h(hdr, dev_image, 16);
        if (hdr[0] == 0 || hdr[0] > 8 || hdr[1] == 0 || hdr[1] > 8 || (image_bytes - 16) % (hdr[0] + hdr[1]))
            throw prim::Error(-22, "bad .rl_bwt header");
        return ImageHeader{hdr[0], hdr[1], (image_bytes - 16) / (hdr[0] + hdr[1])};
    }
    static void check_cell_bytes(int w, const char *who = nullptr) {      // (who: the prefix of the caller's messages, if it has one)
        if (!(w == 1 || w == 2 || w == 4 || w == 8)) throw prim::Error(-22, who ? std::string(who) + ": bad cell width" : std::string("bad cell width"));
    }
    // f(cell_t()) for the cell type of a checked width: `[&](auto c) { typedef decltype(c) cell_t; ... }`
    template <class F>
    static auto with_cell(int cell_bytes, F f) {
        switch (cell_bytes) {
            case 1: return f(u8());
            case 2: return f(u16());
            case 4: return f(u32());
            default: return f(u64());
        }
    }
    // ---- consumers of the .rl_bwt image (validation): grl2plain + reverse_bwt on the device ----------
    // Rebuilds the collection (strings in input order) from an image in device memory.
    // The run symbols of an image are read as 64 bits.  Where the largest is 2^30 or more they are compacted like a wide text
    // (R values, not n): the LF walk runs on ranks and the write functors put alpha[rank] into the text.
    struct WideSyms { DBuf<u32> ranks; DBuf<u64> alpha; };
    static void image_symbols(const ImageRecs &in, u64 R, int cell_bytes, WideSyms &W, const char *who = "inversion") {
        const u64 mx = prim::reduce_max<u64>(R, ImageSymIn{in}, "inv.max_sym");
        if (cell_bytes < 8 && (mx >> (8 * cell_bytes))) throw prim::Error(-22, std::string(who) + ": the image's largest symbol does not fit the cell width");
        if (mx < (1ull << 30)) return;
        DBuf<u64> s64(R);
        prim::for_each(R, UnpackSymFn{in, s64.p}, "inv.unpack_syms");
        W.ranks.alloc(R);
        alphabet_compact<u64>(s64.p, R, mx, W.ranks.p, W.alpha);
    }
    // A record of length zero contributes nothing (the reference's reader, bwt_io.h, just loops over the records; split_runs
    // writes such records in front of a piece that starts on a block boundary).  The consumers that look a POSITION up find its
    // run through one bit per run START, which an empty record would share with its successor -- every later position would
    // read the symbol one record too early.  They drop the empty records first: flag scan + compacting copy, and nothing at
    // all where the shortest record is not empty (every image the engine builds).  Returns the number of records kept.
    // `who` prefixes the labels of the three kernels ("image" or "merge").
    template <class sym_t>
    static u64 drop_empty_runs(DBuf<sym_t> &rsym, DBuf<idx_t> &rlen, u64 R, const char *who = "image") {
        const std::string w(who);
        if (R == 0 || prim::reduce_min<u64>(R, IdxIn64{rlen.p}, (w + ".min_run").c_str()) != 0) return R;
        DBuf<idx_t> dst(R + 1);
        const u64 kept = (u64)prim::exclusive_scan<idx_t>(R, NonEmptyIn{rlen.p}, dst.p, true, (w + ".nonempty").c_str());
        DBuf<sym_t> s2(kept);
        DBuf<idx_t> l2(kept);
        prim::for_each(R, KeepRunsFn<sym_t>{rsym.p, rlen.p, dst.p, s2.p, l2.p}, (w + ".drop_empty").c_str());
        rsym = std::move(s2);
        rlen = std::move(l2);
        return kept;
    }
    template <class T>
    static void d2d_copy(T *dst, const T *src, u64 n) { prim::d2d(dst, src, n * sizeof(T)); }
    // the run-indexed form (functor block "the same inversion indexed by RUNS")
    // The runs of an image as the inverter and the FM index need them.  run_index_load: the non-empty records as arrays, their
    // start positions, the separator and the number of strings.  run_index_lf: the runs in (symbol, position) order and the scan
    // of their lengths in that order -- LF of every run start -- kept in one or both of two forms, after which the arrays go:
    //   walk    rc + rec: the run-start bit-vector with ranks and (LF(start) - start, symbol) per run: LF of any row of the BWT
    //   search  key + slf: (symbol, start) and the scan itself in sorted order: the rank of ANY symbol in front of any row
    struct RunIndex {
        u64 R = 0, n = 0, k = 0;
        u32 sep = 0, mx = 0;
        DBuf<u32> rsym;
        DBuf<idx_t> rlen, rpos;
        DBuf<RankCell> rc;
        DBuf<RunRec> rec;
        DBuf<FmKey> key;
        DBuf<idx_t> slf;
        LfRows lf() const { return LfRows{rc.p, rec.p}; }
    };
    static void run_index_load(const ImageRecs &in, u64 R, const WideSyms &W, RunIndex &X) {
        X.rsym.alloc(R); X.rlen.alloc(R);
        prim::for_each(R, UnpackRunsFn<u32>{in, X.rsym.p, X.rlen.p}, "inv.unpack");
        if (W.alpha.p) d2d_copy(X.rsym.p, W.ranks.p, R);
        X.R = R = drop_empty_runs(X.rsym, X.rlen, R);
        X.rpos.alloc(R + 1);
        X.n = (u64)prim::exclusive_scan<idx_t>(R, IdxIn<idx_t>{X.rlen.p}, X.rpos.p, true, "inv.positions");
        X.sep = prim::reduce_min<u32>(R, PtrU32In{X.rsym.p}, "inv.sep");
        X.mx = prim::reduce_max<u32>(R, PtrU32In{X.rsym.p}, "inv.max");
        X.k = prim::reduce_sum<u64>(R, SepLenIn{X.rsym.p, X.rlen.p, X.sep}, "inv.nstrings");      // strings = separators
    }
    static void run_index_lf(RunIndex &X, bool walk, bool search, bool keep_runs = false) {
        const u64 R = X.R, n = X.n;
        if (walk) {      // run-start bit-vector with the rank of every word beside it
            RankBits rb;
            build_rankbits(rb, X.rpos.p, R, n + 1, "inv.runbits");
            const u64 nw = (n + 1) / 64 + 2;
            X.rc.alloc(nw);
            prim::for_each(nw, RankCellFn{rb.words.p, rb.base.p, X.rc.p}, "inv.rankcells");
            X.rec.alloc(R);
        }
        if (search) { X.key.alloc(R); X.slf.alloc(R + 1); }
        {
            DBuf<u32> k2(R), k3(R);
            DBuf<idx_t> ia(R), ib(R);
            d2d_copy(k2.p, X.rsym.p, R);
            prim::for_each(R, IotaFn{ia.p}, "inv.iota");
            int bits = (int)bitlen64(X.mx);
            if (bits < 1) bits = 1;
            const int res = prim::sort_pairs<u32, idx_t>(k2.p, ia.p, k3.p, ib.p, R, 0, bits, "inv.lf_sort");
            const idx_t *order = res ? ib.p : ia.p;
            const u64 tot = search ? (u64)prim::exclusive_scan_emit<idx_t>(R, RunOrderLenIn{X.rlen.p, order}, FmKeyEmitFn{order, X.rpos.p, X.rsym.p, X.rec.p, X.key.p, X.slf.p}, "fm.keys")
                                   : (u64)prim::exclusive_scan_emit<idx_t>(R, RunOrderLenIn{X.rlen.p, order}, RunLfEmitFn{order, X.rpos.p, X.rsym.p, X.rec.p}, "inv.lf");
            if (tot != n) throw prim::Error(-71, "inversion: run lengths do not add up");
        }
        if (search) { const idx_t total = (idx_t)n; prim::h2d(X.slf.p + R, &total, sizeof(total)); }
        if (!keep_runs) { X.rsym.release(); X.rlen.release(); X.rpos.release(); }
    }
    // the position-indexed form: the BWT expanded to one symbol per position, LF as an array over them
    template <class cell_t>
    static u64 invert_t(const ImageRecs &in, u64 R, cell_t *text_out, u64 capacity, const WideSyms &W) {
        RunIndex X;
        run_index_load(in, R, W, X);
        const u64 n = X.n, k = X.k;
        const u32 sep = X.sep;
        if (n > capacity) throw prim::Error(-22, "inversion: output buffer too small");
        RankBits rb;
        build_rankbits(rb, X.rpos.p, X.R, n + 1, "inv.runbits");
        DBuf<u32> bwt(n), k2(n);
        DBuf<idx_t> ia(n), ib(n), lf(n);
        prim::for_each(n, ExpandRunsFn{X.rsym.p, rb.words.p, rb.base.p, bwt.p, ia.p}, "inv.expand");          // grl2plain
        d2d_copy(k2.p, bwt.p, n);
        DBuf<u32> k3(n);
        const int res = prim::sort_pairs<u32, idx_t>(k2.p, ia.p, k3.p, ib.p, n, 0, std::max((int)bitlen64(X.mx), 1), "inv.lf_sort");
        prim::for_each(n, LfScatterFn{res ? ib.p : ia.p, lf.p}, "inv.lf");
        k2.release(); k3.release();
        DBuf<idx_t> slen(k + 1);
        prim::for_each(k, InvertLenFn{bwt.p, lf.p, sep, slen.p}, "inv.lengths");
        const u64 tot = (u64)prim::exclusive_scan<idx_t>(k, IdxIn<idx_t>{slen.p}, slen.p, true, "inv.offsets");
        if (tot != n) throw prim::Error(-71, "inversion: string lengths do not add up to the BWT length");
        prim::for_each(k, InvertWriteFn<cell_t>{bwt.p, lf.p, slen.p, sep, text_out, {W.alpha.p}}, "inv.write");
        prim::sync();
        return n;
    }
    template <class cell_t>
    static u64 invert_runs_t(const ImageRecs &in, u64 R, cell_t *text_out, u64 capacity, const WideSyms &W, u64 tail = 0, u64 *n_strings_out = nullptr) {
        RunIndex X;
        run_index_load(in, R, W, X);
        const u64 n = X.n;
        if (!tail && n > capacity) throw prim::Error(-22, "inversion: output buffer too small");
        run_index_lf(X, true, false);
        const u64 k = X.k;
        const u32 sep = X.sep;
        const LfRows lf = X.lf();
        if (tail) {
            // the ends of the strings only (collections whose strings are too long to walk in a test's time -- 100
            // strings of 249 M cells are 249 M dependent steps each): `tail` LF steps per string from its terminator's row
            if (k * tail > capacity) throw prim::Error(-22, "inversion: output buffer too small");
            DBuf<idx_t> got(k);
            prim::for_each(k, RunInvertTailFn<cell_t>{lf, sep, tail, text_out, got.p, {W.alpha.p}}, "inv.tails");
            prim::sync();
            if (n_strings_out) *n_strings_out = k;
            return (u64)prim::reduce_sum<u64>(k, IdxIn<idx_t>{got.p}, "inv.tails");
        }
        DBuf<idx_t> slen(k + 1);
        prim::for_each(k, RunInvertLenFn{lf, sep, slen.p}, "inv.lengths");
        const u64 tot = (u64)prim::exclusive_scan<idx_t>(k, IdxIn<idx_t>{slen.p}, slen.p, true, "inv.offsets");
        if (tot != n) throw prim::Error(-71, "inversion: string lengths do not add up to the BWT length");
        prim::for_each(k, RunInvertWriteFn<cell_t>{lf, slen.p, sep, text_out, {W.alpha.p}}, "inv.write");
        prim::sync();
        return n;
    }

    // ---- checkpointed LF walks (functor block "checkpointed LF walks") -------------------------------------
    // lf_checkpoints: phases A and B on the rc + rec arrays run_index_lf(X, true, ...) makes.  Scratch: six idx_t arrays of m
    // (seglen, next, two generations of (ptr, acc)) and two per string.  On return head[c] / dist[c] are c's string and the LF
    // steps from that string's end row to c, slen[i] is the length of string i (separator included) and endcp[j] the checkpoint
    // whose segment ends at the j-th separator.
    //   Loops: the segment walks are bounded by n steps each; the pointer jumping runs a counted number of rounds, at most
    //   ceil(log2 m), and ends early when a reduce says that no pointer moved; nothing waits for another thread.
    struct WalkInfo { u64 k = 0, m = 0, b = 0, longest_segment = 0, longest_chain = 0, jump_rounds = 0, lanes = 0, refills = 0, scratch_bytes = 0, sample_bytes = 0; };
    static constexpr bool kWalkPackedStores(char sw) { return sw != 'c'; }      // the store form of the write walk: words won
    static constexpr int kDefaultSampleBits = 8;      // what sample_bits = 0 means
    static int sample_bits_of(int b) {
        if (b < 0 || b > 20) throw prim::Error(-22, "checkpointed walk: sample_bits is 0 (the default) or 1 to 20");
        return b ? b : kDefaultSampleBits;
    }
    struct CpRank {
        Checkpoints cp{0, 0, 0};
        DBuf<idx_t> seglen, next, head, dist, ptr2, acc2, endcp, slen;
    };
    template <class F>
    static void walk(u64 m, F f, WalkInfo &wi, const char *name) {
#ifdef GRLBWT_PRIM_HIP
        DBuf<u64> ctr(2);
        const prim::WalkStats ws = prim::walk_tickets(m, f, ctr.p, name);
        wi.lanes = ws.lanes; wi.refills = ws.refills;
#else
        prim::for_each(m, WalkSerialFn<F>{f}, name);
        wi.lanes = m; wi.refills = 0;
#endif
    }
    static void lf_checkpoints(const LfRows &lf, u64 n, u64 k, u32 sep, int b, int bad_code, CpRank &C, WalkInfo &wi) {
        const Checkpoints cp{n, k, (u32)b};
        const u64 m = cp.count();
        if (m >= (u64)kCpEnd) throw prim::Error(-75, "checkpointed walk: more checkpoints than positions of this width can number");
        C.cp = cp;
        wi.k = k; wi.m = m; wi.b = (u64)b;
        wi.scratch_bytes = (6 * m + 2 * k + 1) * sizeof(idx_t) + k * 8;
        C.seglen.alloc(m); C.next.alloc(m); C.head.alloc(m); C.dist.alloc(m); C.ptr2.alloc(m); C.acc2.alloc(m);
        C.endcp.alloc(k); C.slen.alloc(k + 1);
        DBuf<u32> bad(1);
        bad.zero();
        walk(m, CpSegFn{lf, sep, cp, C.seglen.p, C.next.p, C.endcp.p, bad.p}, wi, "cp.segments");
        if (bad.get(0)) throw prim::Error(bad_code, "checkpointed walk: a segment met no checkpoint in n steps: not the BWT of a collection");
        wi.longest_segment = prim::reduce_max<u64>(m, IdxIn64{C.seglen.p}, "cp.longest");
        prim::for_each(m, CpInitFn{k, C.head.p, C.dist.p}, "cp.init");
        prim::for_each(m, CpPrevFn{C.next.p, C.seglen.p, C.head.p, C.dist.p}, "cp.prev");
        const u64 cap = m > 1 ? (u64)bitlen64(m - 1) : 0;       // ceil(log2 m)
        for (u64 r = 0; r < cap; r++) {
            prim::for_each(m, CpJumpFn{C.head.p, C.dist.p, C.ptr2.p, C.acc2.p}, "cp.jump");
            wi.jump_rounds++;
            const u64 moved = prim::reduce_sum<u64>(m, CpMovedIn{C.head.p, C.ptr2.p}, "cp.moved");
            std::swap(C.head, C.ptr2);
            std::swap(C.dist, C.acc2);
            if (!moved) break;
        }
        C.ptr2.release(); C.acc2.release(); C.next.release();
        DBuf<u64> chain(k);
        chain.zero();
        prim::for_each(m, CpHeadFn{k, C.head.p, chain.p}, "cp.heads");
        wi.longest_chain = prim::reduce_max<u64>(k, CellIn<u64>{chain.p}, "cp.chains");
        C.slen.zero();
        prim::for_each(k, CpLenFn{C.endcp.p, C.head.p, C.dist.p, C.seglen.p, C.slen.p, bad.p}, "cp.lengths");
        if (bad.get(0)) throw prim::Error(bad_code, "checkpointed walk: a string's end lies on no string's chain: not the BWT of a collection");
    }
    template <class cell_t>
    static u64 invert_checkpointed_t(const ImageRecs &in, u64 R, cell_t *text_out, u64 capacity, const WideSyms &W, int b, WalkInfo &wi) {
        RunIndex X;
        run_index_load(in, R, W, X);
        const u64 n = X.n;
        if (n > capacity) throw prim::Error(-22, "inversion: output buffer too small");
        run_index_lf(X, true, false);
        CpRank C;
        lf_checkpoints(X.lf(), n, X.k, X.sep, b, -71, C, wi);
        const u64 tot = (u64)prim::exclusive_scan<idx_t>(X.k, IdxIn<idx_t>{C.slen.p}, C.slen.p, true, "inv.offsets");
        if (tot != n) throw prim::Error(-71, "inversion: string lengths do not add up to the BWT length");
        const CpWriteFn<cell_t> wf{X.lf(), X.sep, C.cp, C.head.p, C.dist.p, C.seglen.p, C.slen.p, text_out, {W.alpha.p}};
        bool packed = false;
        if constexpr (sizeof(cell_t) <= 2) packed = kWalkPackedStores(prim::sw().dev_walk_stores) && ((uintptr_t)text_out & 7) == 0;
        if constexpr (sizeof(cell_t) <= 2) { if (packed) walk(wi.m, CpWritePackedFn<cell_t>{wf}, wi, "cp.write_packed"); }
        if (!packed) walk(wi.m, wf, wi, "cp.write");
        prim::sync();
        return n;
    }
    static u64 invert_image_checkpointed(const void *dev_image, u64 image_bytes, int cell_bytes, int sample_bits, void *dev_text_out, u64 capacity_cells, WalkInfo &wi) {
        const int b = sample_bits_of(sample_bits);
        const ImageHeader h = image_header(dev_image, image_bytes);
        const ImageRecs in = h.recs(dev_image);
        check_cell_bytes(cell_bytes);
        WideSyms W;
        image_symbols(in, h.R, cell_bytes, W);
        return with_cell(cell_bytes, [&](auto c) {
            typedef decltype(c) cell_t;
            return invert_checkpointed_t<cell_t>(in, h.R, (cell_t *)dev_text_out, capacity_cells, W, b, wi);
        });
    }

    // the last `tail` cells of every string (slot i of `tail` cells holds string i's end, right-aligned); returns the cells written
    static u64 invert_image_tails(const void *dev_image, u64 image_bytes, int cell_bytes, u64 tail, void *dev_out, u64 capacity_cells, u64 *n_strings_out) {
        if (image_bytes < 16 || tail == 0) throw prim::Error(-22, "not an .rl_bwt image, or no tail length");
        const ImageHeader h = image_header(dev_image, image_bytes);
        const ImageRecs in = h.recs(dev_image);
        check_cell_bytes(cell_bytes);
        WideSyms W;
        image_symbols(in, h.R, cell_bytes, W);
        return with_cell(cell_bytes, [&](auto c) {
            typedef decltype(c) cell_t;
            return invert_runs_t<cell_t>(in, h.R, (cell_t *)dev_out, capacity_cells, W, tail, n_strings_out);
        });
    }

    static u64 invert_image(const void *dev_image, u64 image_bytes, int cell_bytes, void *dev_text_out, u64 capacity_cells, u64 n_total_hint = 0) {
        const ImageHeader h = image_header(dev_image, image_bytes);
        const ImageRecs in = h.recs(dev_image);
        check_cell_bytes(cell_bytes);
        WideSyms W;
        image_symbols(in, h.R, cell_bytes, W);
        // Two index forms.  Per POSITION (LF array: one gather per symbol of a string, (12 + 3 * sizeof(idx_t)) bytes per symbol
        // while it is built) when that fits the device comfortably; per RUN (two dependent gathers per symbol, 30-50 bytes per
        // run) otherwise -- the 10 GB headline image needs 360 GB in the first form and ~100 GB in the second.
        // GRLBWT_INVERT=runs|positions forces one (the tests take both on small inputs).
        bool by_runs = (n_total_hint ? n_total_hint : capacity_cells) * (12 + 3 * (u64)sizeof(idx_t)) > prim::mem_available() / 2;
        if (prim::sw().invert) by_runs = prim::sw().invert == 'r';
        return with_cell(cell_bytes, [&](auto c) {
            typedef decltype(c) cell_t;
            return by_runs ? invert_runs_t<cell_t>(in, h.R, (cell_t *)dev_text_out, capacity_cells, W) : invert_t<cell_t>(in, h.R, (cell_t *)dev_text_out, capacity_cells, W);
        });
    }

    // ---- the FM index over the runs of an image (grlbwt_fm_*; functor block "counting and locating patterns") ----------------
    struct ExtractInfo { u64 ranges = 0, pieces = 0, cells = 0, steps = 0, lanes = 0, refills = 0; };      // of the last fm_extract
    struct MatchInfo { u64 patterns = 0, cells = 0, matched = 0, longest = 0, capped = 0, mems = 0, lanes = 0, refills = 0; };
    struct ApproxInfo { u64 patterns = 0, cells = 0, k = 0, max_hits = 0, hits = 0, by[4] = {0, 0, 0, 0}, cut = 0, steps = 0, lanes = 0, refills = 0; };
    struct LcpInfo { u64 n = 0, k = 0, lcp_bytes = 0, cap = 0, passes = 0, n_levels = 0, max_lcp = 0, n_capped = 0, tile_rows = 0, scratch_bytes = 0; };      // of the last fm_lcp
    struct SaInfo {           // of the last fm_sa
        u64 n = 0, k = 0, row_begin = 0, row_end = 0, string_bytes = 0, offset_bytes = 0, written = 0, form = 0, steps = 0, longest = 0, lanes = 0, refills = 0,
            scratch_bytes = 0;
    };
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kOverlapTile = prim::kExpandTile;
#else
    static constexpr u64 kOverlapTile = 2048;    // (the serial form has no tiles: the figure the device library reports)
#endif
    struct OverlapInfo {      // of the last fm_overlaps / fm_overlaps_of (the first eight) or fm_overlap_targets (ranges, entries)
        u64 patterns = 0, cells = 0, hits = 0, targets = 0, longest = 0, steps = 0, lanes = 0, refills = 0, ranges = 0, entries = 0, tile = kOverlapTile;
    };
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kKmerTileRows = prim::kKmerTile, kKmerTileEntries = prim::kKmerEntries, kKmerStageBytes = prim::kKmerStage;
#else
    static constexpr u64 kKmerTileRows = 4096, kKmerTileEntries = 256, kKmerStageBytes = 16384;      // (the serial form has no tiles: the figures the device library reports)
#endif
    static constexpr u64 kKmerMaxBins = 16384;
    struct KmerInfo {         // of the last fm_kmers that got as far as counting
        u64 k = 0, n = 0, n_strings = 0, n_distinct = 0, n_windows = 0, n_selected = 0, largest_count = 0, passes = 0, length_passes = 0, forward_steps = 0;
        u64 tile_rows = kKmerTileRows, tile_kmers = kKmerTileEntries, stage_bytes = kKmerStageBytes, scratch_bytes = 0;
    };
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kCkMateTile = prim::kTopThreads;
#else
    static constexpr u64 kCkMateTile = 1024;     // (the serial form has no tiles: the figure the device library reports)
#endif
    struct CkmerInfo {        // of the last fm_ckmers that got as far as counting
        u64 k = 0, n = 0, n_strings = 0, n_distinct = 0, n_windows = 0, n_selected = 0, n_classes = 0, n_paired = 0, n_palindromes = 0, n_single = 0,
            n_no_complement = 0, largest_total = 0, passes = 0, length_passes = 0, mate_walks = 0, backward_steps = 0, forward_steps = 0;
        u64 tile_rows = kKmerTileRows, tile_kmers = kKmerTileEntries, mate_tile = kCkMateTile, stage_bytes = kKmerStageBytes, scratch_bytes = 0;
    };
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kRepTileRows = prim::kRepTile;
#else
    static constexpr u64 kRepTileRows = kRepFanout * kRepFanout;      // (the serial form has no tiles: the figure the device library reports)
#endif
    struct RepeatInfo {       // of the last fm_repeats that got as far as counting
        u64 n = 0, n_strings = 0, min_len = 0, max_len = 0, passes = 0, n_repeats = 0, n_maximal = 0, n_selected = 0, longest = 0, largest_count = 0;
        u64 value_bytes = 0, tile_rows = kRepTileRows, tree_fanout = kRepFanout, tree_levels = 0, far_searches = 0, scratch_bytes = 0;
    };
    struct FmIndex {
        u64 n = 0, R = 0, k = 0, sigma = 0, sepval = 0;
        u32 sep = 0, top_entries = 0;
        bool locate = false;
        DBuf<FmKey> key;
        DBuf<idx_t> slf;
        DBuf<u64> alpha;          // the values of a compacted alphabet (null: the symbols are the values)
        DBuf<RankCell> rc;        // locate: LF of any row (LfRows) and the string behind every separator
        DBuf<RunRec> rec;
        DBuf<idx_t> sid;
        LfRows lf() const { return LfRows{rc.p, rec.p}; }
        bool checkpoints = false; // locate with samples: (string, offset) of every checkpoint row, two idx_t each
        Checkpoints cp{0, 0, 0};
        DBuf<idx_t> smp;
        WalkInfo walk;
        bool extract = false;     // extract: the strings' start positions T (k + 1) and the inverse of the samples, (position, checkpoint) by position
        u64 maxval = 0;           // (the largest symbol's value)
        DBuf<idx_t> T, xq, xc;
        mutable ExtractInfo xinfo;
        mutable MatchInfo minfo;  // of the last fm_match / fm_mems
        mutable ApproxInfo ainfo; // of the last fm_approx
        mutable LcpInfo linfo;    // of the last fm_lcp
        mutable SaInfo sinfo;     // of the last fm_sa
        mutable KmerInfo kinfo;   // of the last fm_kmers that got as far as counting
        mutable CkmerInfo cinfo;  // of the last fm_ckmers that got as far as counting
        mutable RepeatInfo rinfo; // of the last fm_repeats that got as far as counting
        mutable OverlapInfo oinfo; // of the last fm_overlaps, fm_overlaps_of or fm_overlap_targets
        u64 extract_bytes() const { return (T.n + xq.n + xc.n) * sizeof(idx_t); }
        u64 bytes() const {
            return key.n * sizeof(FmKey) + slf.n * sizeof(idx_t) + alpha.n * 8 + rc.n * sizeof(RankCell) + rec.n * sizeof(RunRec) + sid.n * sizeof(idx_t) +
                   smp.n * sizeof(idx_t) + extract_bytes();
        }
    };
    // What the locate structures may take while they are made: half of the free device memory (a quarter byte per symbol for the
    // bit-vector and its ranks, a word per string).  The serial stand-in, which walks the strings one after the other, stops at 256 MB.
    static u64 fm_locate_budget() { return prim::kIsDevice ? prim::mem_available() / 2 : (u64)1 << 28; }
    static void fm_create(const void *dev_image, u64 image_bytes, bool locate, int top_bits, FmIndex &F, bool checkpoints = false, int sample_bits = 0,
                          bool extract = false) {
        if (extract && !locate) throw prim::Error(-22, "fm index: extracting needs the structures for locating");
        const int b = checkpoints ? sample_bits_of(sample_bits) : 0;
        const ImageHeader h = image_header(dev_image, image_bytes);
        if (h.R == 0) throw prim::Error(-22, "fm index: the image has no record");
        if (top_bits < 0 || top_bits > 12) throw prim::Error(-22, "fm index: the top level takes 0 to 12 bits");
        WideSyms W;
        image_symbols(h.recs(dev_image), h.R, 8, W);
        RunIndex X;
        run_index_load(h.recs(dev_image), h.R, W, X);
        W.ranks.release();
        F.n = X.n; F.R = X.R; F.k = X.k; F.sep = X.sep; F.locate = locate;
        if (locate) {
            const u64 words = (X.n + 1) / 64 + 2;
            u64 need = words * (sizeof(RankCell) + 8 + sizeof(idx_t)) + X.R * sizeof(RunRec) + X.k * sizeof(idx_t);
            if (checkpoints) need += (Checkpoints{X.n, X.k, (u32)b}.count() * 8 + 2 * X.k + 1) * sizeof(idx_t) + X.k * 8;       // the ranking's scratch and the samples
            // the inverse table (a pair per sample, at most one per checkpoint) beside the second half of its sort, and T
            if (extract) need += (4 * (checkpoints ? Checkpoints{X.n, X.k, (u32)b}.count() : X.k) + X.k + 1) * sizeof(idx_t);
            if (X.n >= ((u64)1 << 62) || need > fm_locate_budget())
                throw prim::Error(-22, "fm index: the structures for locating (" + std::to_string(need) + " bytes) are more than this device can hold");
        }
        run_index_lf(X, locate && X.R, true);
        F.key = std::move(X.key); F.slf = std::move(X.slf); F.rc = std::move(X.rc); F.rec = std::move(X.rec);
        F.alpha = std::move(W.alpha);
        F.sigma = prim::reduce_sum<u64>(F.R, FmHeadIn{F.key.p}, "fm.sigma");
        if (F.R) F.sepval = F.alpha.p ? F.alpha.get(F.sep) : (u64)F.sep;
#ifdef GRLBWT_PRIM_HIP
        F.top_entries = prim::top_search_entries(top_bits, F.R, sizeof(FmKey));
#endif
        if (locate && F.R && checkpoints) {
            // sid from the chain ends (FmSidLenFn is not run) and the samples.  An image with rows on no string's chain (cycles of LF
            // without a separator) is accepted as without checkpoints: such rows have no position, their samples say so.
            CpRank C;
            lf_checkpoints(F.lf(), F.n, F.k, F.sep, b, -22, C, F.walk);
            F.checkpoints = true;
            F.cp = C.cp;
            F.sid.alloc(F.k);
            prim::for_each(F.k, CpSidFn{C.endcp.p, C.head.p, F.sid.p}, "fm.sid_chains");
            F.smp.alloc(2 * F.walk.m);
            prim::for_each(F.walk.m, CpSampleFn{C.head.p, C.dist.p, C.slen.p, F.smp.p}, "fm.samples");
            F.walk.sample_bytes = F.smp.n * sizeof(idx_t);
            if (extract) {
                const u64 m = F.walk.m;
                C.seglen.release(); C.endcp.release();
                F.T.alloc(F.k + 1);
                prim::exclusive_scan<idx_t>(F.k, IdxIn<idx_t>{C.slen.p}, F.T.p, true, "fm.extract_starts");
                DBuf<idx_t> ka(m), va(m), kb(m), vb(m);
                prim::for_each(m, FmCpSampleKeyFn{C.cp, C.head.p, C.dist.p, F.T.p, ka.p, va.p}, "fm.extract_keys");
                C.head.release(); C.dist.release();
                const u64 ns = prim::reduce_sum<u64>(m, FmSampleValidIn{ka.p, F.n}, "fm.extract_samples");
                const int res = prim::sort_pairs<idx_t, idx_t>(ka.p, va.p, kb.p, vb.p, m, 0, std::max((int)bitlen64(F.n), 1), "fm.extract_sort");
                F.xq.alloc(ns); F.xc.alloc(ns);      // (the ns samples come first: the others carry n)
                d2d_copy(F.xq.p, res ? kb.p : ka.p, ns);
                d2d_copy(F.xc.p, res ? vb.p : va.p, ns);
            }
        } else if (locate && F.R && extract) {
            DBuf<u32> bad(1);
            bad.zero();
            F.sid.alloc(F.k);
            DBuf<idx_t> slen(F.k + 1);
            slen.zero();
            prim::for_each(F.k, FmSidLenFn{F.lf(), F.sep, F.n, F.sid.p, slen.p, bad.p}, "fm.sid_len");
            if (bad.get(0)) throw prim::Error(-22, "fm index: a string's walk met no separator in n steps: not the BWT of a collection");
            F.cp = Checkpoints{F.n, F.k, 0};         // (row_of(c) = c below k: the heads' rows)
            F.T.alloc(F.k + 1);
            prim::exclusive_scan<idx_t>(F.k, IdxIn<idx_t>{slen.p}, F.T.p, true, "fm.extract_starts");
            F.xq.alloc(F.k); F.xc.alloc(F.k);
            prim::for_each(F.k, FmHeadSampleFn{F.T.p, F.xq.p, F.xc.p}, "fm.extract_heads");
        } else if (locate && F.R) {
            DBuf<u32> bad(1);
            bad.zero();
            F.sid.alloc(F.k);
            prim::for_each(F.k, FmSidLenFn{F.lf(), F.sep, F.n, F.sid.p, nullptr, bad.p}, "fm.sid");
            if (bad.get(0)) throw prim::Error(-22, "fm index: a string's walk met no separator in n steps: not the BWT of a collection");
        }
        if (extract) { F.extract = true; F.maxval = F.alpha.p ? F.alpha.get(F.alpha.n - 1) : (u64)X.mx; }
        prim::sync();
    }
    // the checks every call that takes patterns shares; returns the number of their cells, the first one's index in `x0`
    static u64 fm_match_cells(const void *cells, int w, const u64 *off, u64 np, u64 &x0, const char *who) {
        check_cell_bytes(w, who);
        x0 = 0;
        if (np == 0) return 0;
        if (prim::reduce_sum<u64>(np, FmOffsetsBadIn{off}, "fm.offsets")) throw prim::Error(-22, std::string(who) + ": the pattern offsets decrease");
        u64 x1;
        prim::d2h(&x0, off, 8);
        prim::d2h(&x1, off + np, 8);
        if (x1 > x0 && !cells) throw prim::Error(-22, std::string(who) + ": no pattern cells");
        return x1 - x0;
    }
    static FmCountFn fm_count_fn(const FmIndex &F, const void *cells, int w, const u64 *off, u64 *lo, u64 *hi) {
        return FmCountFn{F.key.p, F.slf.p, F.R, F.n, F.alpha.p, F.alpha.n, cells, w, off, lo, hi};
    }
    static void fm_count(const FmIndex &F, const void *cells, int w, const u64 *off, u64 np, u64 *lo, u64 *hi) {
        u64 x0;
        const u64 nc = fm_match_cells(cells, w, off, np, x0, "fm count");
        if (np == 0) return;
        const FmCountFn f = fm_count_fn(F, cells, w, off, lo, hi);
        if (F.R) {
            // the separator ends a string: a pattern may END with it (the step from [0, n) gives [0, n_strings), the rows of
            // the strings' ends) but the rows a further step would lead to are no range of a BCR BWT
            const u64 bad = prim::reduce_min<u64>(nc, FmSepMisuseIn{f, F.sepval, x0, np}, "fm.separators");
            if (bad != ~0ull) throw prim::Error(-22, "fm count: pattern " + std::to_string(bad) + " holds the separator in front of its last cell");
        }
#ifdef GRLBWT_PRIM_HIP
        prim::top_search(np, f, F.top_entries, "fm.count");
#else
        prim::for_each(np, FmCountPlainFn{f}, "fm.count");
#endif
        prim::sync();
    }
    // ---- longest matches and MEMs (functor block "longest matches and maximal exact matches").  Everything that
    // can refuse a call runs before the first store into an output.  One ticket per query cell; the device form is
    // prim::top_tickets (lanes that take the next cell when their match ends, under the LDS top level of fm_count), or with
    // GRLBWT_FM_MATCH=l one lane per cell through prim::top_search; the stand-in runs the same functor serially.
    //   The compiler's report for gfx950 (tools/kernel_resources.py): prim::k_top_tickets<FmMatchFn> takes 46 vector registers in
    //   both index widths (k_top_search<FmMatchLaneFn> 32, k_top_search<FmCountFn> 26), no scratch, no static LDS -- the dynamic
    //   LDS is the top level, at most 32 KB of 8-byte keys or 64 KB of 16-byte keys; 8 waves per SIMD fit either way.
    static void fm_match_run(const FmIndex &F, const FmMatchFn &f, u64 nc, u64 np, MatchInfo &mi) {
        mi = MatchInfo();
        mi.patterns = np; mi.cells = nc;
        if (nc == 0) return;
#ifdef GRLBWT_PRIM_HIP
        if (prim::sw().fm_match == 'l') {
            prim::top_search(nc, FmMatchLaneFn{f}, F.top_entries, "fm.match_lanes");
            mi.lanes = nc;
        } else {
            DBuf<u64> ctr(2);
            const prim::WalkStats ws = prim::top_tickets(nc, f, ctr.p, F.top_entries, "fm.match");
            mi.lanes = ws.lanes; mi.refills = ws.refills;
        }
#else
        prim::for_each(nc, WalkSerialFn<FmMatchFn>{f}, "fm.match");
        mi.lanes = nc;
#endif
        mi.matched = prim::reduce_sum<u64>(nc, CellIn<u64>{f.len}, "fm.match_sum");
        mi.longest = prim::reduce_max<u64>(nc, CellIn<u64>{f.len}, "fm.match_max");
        if (f.max_len) mi.capped = prim::reduce_sum<u64>(nc, FmLenCappedIn{f.len, f.max_len}, "fm.match_capped");
    }
    static FmMatchFn fm_match_fn(const FmIndex &F, const void *cells, int w, const u64 *off, u64 np, u64 x0, u64 max_len, u64 *len, u64 *lo, u64 *hi) {
        return FmMatchFn{fm_count_fn(F, cells, w, off, nullptr, nullptr), F.sepval, x0, np, max_len, len, lo, hi};
    }
    static void fm_match(const FmIndex &F, const void *cells, int w, const u64 *off, u64 np, u64 max_len, u64 *len, u64 *lo, u64 *hi) {
        if ((lo == nullptr) != (hi == nullptr)) throw prim::Error(-22, "fm match: the range outputs are both given or both null");
        u64 x0;
        const u64 nc = fm_match_cells(cells, w, off, np, x0, "fm match");
        if (nc && !len) throw prim::Error(-22, "fm match: no output for the lengths");
        MatchInfo mi;
        fm_match_run(F, fm_match_fn(F, cells, w, off, np, x0, max_len, len, lo, hi), nc, np, mi);
        prim::sync();
        F.minfo = mi;
    }
    // n_mems is set whenever the count was reached, also when the capacity then refuses the call
    static void fm_mems(const FmIndex &F, const void *cells, int w, const u64 *off, u64 np, u64 min_len, u64 max_len, u64 *pat, u64 *beg, u64 *mlen,
                        u64 *lo, u64 *hi, u64 capacity, u64 &n_mems) {
        n_mems = 0;
        if ((lo == nullptr) != (hi == nullptr)) throw prim::Error(-22, "fm mems: the range outputs are both given or both null");
        u64 x0;
        const u64 nc = fm_match_cells(cells, w, off, np, x0, "fm mems");
        MatchInfo mi;
        mi.patterns = np;
        if (nc == 0) { prim::sync(); F.minfo = mi; return; }
        const u64 nw = nc / 64 + 2;
        const u64 need = nc * 8 * (lo ? 3 : 1) + nw * 16 + 24;
        if (need > prim::mem_available()) throw prim::Error(-12, "fm mems: the scratch needs " + std::to_string(need) + " bytes of device memory, more than is free");
        DBuf<u64> L(nc), slo(lo ? nc : 0), shi(lo ? nc : 0), words(nw), base(nw + 1);
        fm_match_run(F, fm_match_fn(F, cells, w, off, np, x0, max_len, L.p, lo ? slo.p : nullptr, lo ? shi.p : nullptr), nc, np, mi);
        words.zero();
        prim::bitvector_from_pred(nc, FmMemFlagIn{L.p, off, x0, np, min_len ? min_len : 1}, words.p, "fm.mem_flags");
        mi.mems = n_mems = prim::exclusive_scan<u64>(nw, PopcIn{words.p}, base.p, true, "fm.mem_ranks");
        if (n_mems > capacity)
            throw prim::Error(-22, "fm mems: " + std::to_string(n_mems) + " matches, more than the output arrays hold");
        if (n_mems && (!pat || !beg || !mlen)) throw prim::Error(-22, "fm mems: no output arrays");
        prim::for_each_set_bit<u64>(nc, words.p, base.p, FmMemEmitFn{L.p, slo.p, shi.p, off, x0, np, pat, beg, mlen, lo, hi}, "fm.mems");
        prim::sync();
        F.minfo = mi;
    }
    // ---- patterns with up to k substituted cells (functor block "patterns with up to k substituted cells").
    // Everything that can refuse the call runs before the first store into an output: the count pass writes scratch only (one word
    // per pattern), its sum is held against the capacity, then the scan writes dev_hit_offsets and the emit pass the entries.  One
    // ticket per pattern through prim::top_tickets -- neighbouring patterns differ by orders of magnitude in cost, a lane whose
    // search has ended takes the next pattern -- or with GRLBWT_FM_MATCH=l one lane per pattern through prim::top_search; the
    // stand-in runs the same functor serially.
    //   The compiler's report for gfx950 (tools/kernel_resources.py; profiles/fm_approx/kernel_resources.txt):
    //   k_top_tickets<FmApproxFn> 95 VGPRs, 5 waves per SIMD; k_top_search<FmApproxLaneFn> 67 / 66 (32- / 64-bit positions), 7 waves; no scratch in either.
    static void fm_approx_run(const FmIndex &F, const FmApproxFn &f, u64 np, ApproxInfo &ai) {
#ifdef GRLBWT_PRIM_HIP
        if (prim::sw().fm_match == 'l') {
            prim::top_search(np, FmApproxLaneFn{f}, F.top_entries, "fm.approx_lanes");
            ai.lanes = np; ai.refills = 0;
        } else {
            DBuf<u64> ctr(2);
            const prim::WalkStats ws = prim::top_tickets(np, f, ctr.p, F.top_entries, "fm.approx");
            ai.lanes = ws.lanes; ai.refills = ws.refills;
        }
#else
        prim::for_each(np, WalkSerialFn<FmApproxFn>{f}, "fm.approx");
        ai.lanes = np; ai.refills = 0;
#endif
    }
    static constexpr u32 kApproxMaxK = 3;
    // n_hits is set whenever the count was reached, also when the capacity then refuses the call
    static void fm_approx(const FmIndex &F, const void *cells, int w, const u64 *off, u64 np, u32 k, u64 max_hits, u64 *hoff, u64 *mism, u64 *lo, u64 *hi,
                          u64 *spos, u64 *sval, u64 capacity, u64 &n_hits) {
        n_hits = 0;
        if (k > kApproxMaxK) throw prim::Error(-22, "fm approx: at most 3 substitutions");
        if ((spos == nullptr) != (sval == nullptr)) throw prim::Error(-22, "fm approx: the substitution outputs are both given or both null");
        u64 x0;
        const u64 nc = fm_match_cells(cells, w, off, np, x0, "fm approx");
        ApproxInfo ai;
        ai.patterns = np; ai.cells = nc; ai.k = k; ai.max_hits = max_hits;
        if (np == 0) {
            if (hoff) prim::dev_memset(hoff, 0, 8);
            prim::sync();
            F.ainfo = ai;
            return;
        }
        if (np >= (~0ull >> 4) || (np + 1) * 8 + 64 > prim::mem_available())
            throw prim::Error(-12, "fm approx: the counts need " + std::to_string((np + 1) * 8) + " bytes of device memory, more than is free");
        DBuf<u64> cnt(np + 1);
        DBuf<u32> bad(1);
        bad.zero();
        FmApproxFn f{fm_count_fn(F, cells, w, off, nullptr, nullptr), F.sep, F.sepval, k, max_hits, cnt.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bad.p};
        fm_approx_run(F, f, np, ai);
        ai.hits = n_hits = prim::reduce_sum<u64>(np, FmApproxHitsIn{cnt.p}, "fm.approx_hits");
        ai.cut = prim::reduce_sum<u64>(np, FmApproxCutIn{cnt.p}, "fm.approx_cut");
        if (n_hits > capacity) throw prim::Error(-22, "fm approx: " + std::to_string(n_hits) + " hits, more than the output arrays hold");
        if (!hoff || (n_hits && (!mism || !lo || !hi))) throw prim::Error(-22, "fm approx: no output arrays");      // (the sizing call takes none)
        prim::exclusive_scan<u64>(np, FmApproxHitsIn{cnt.p}, hoff, true, "fm.approx_offsets");
        // (without a hit the arrays may be missing: the pass then stores no entry, and the spare scratch word marks it as the emit pass)
        f.hoff = hoff; f.mism = mism ? mism : cnt.p + np; f.lo = lo; f.hi = hi; f.spos = k ? spos : nullptr; f.sval = k ? sval : nullptr;
        fm_approx_run(F, f, np, ai);
        if (bad.get(0)) throw prim::Error(-71, "fm approx: a pattern's second pass found another number of hits than its first");
        ai.steps = prim::reduce_sum<u64>(np, CellIn<u64>{cnt.p}, "fm.approx_steps");
        for (u32 d = 0; d <= k && n_hits; d++) ai.by[d] = prim::reduce_sum<u64>(n_hits, FmApproxMismIn{mism, (u64)d}, "fm.approx_strata");
        prim::sync();
        F.ainfo = ai;
    }
    // ---- suffix-prefix overlaps (functor block "suffix-prefix overlaps").  Everything that can refuse a call runs
    // before the first store into an output: the count pass writes scratch only (one word per query), its sum is held against the
    // capacity, then the scan writes dev_hit_offsets and the emit pass the entries.  One ticket per query through
    // prim::top_tickets -- a read with an error ends after a few cells, its neighbour runs to its first cell -- or with
    // GRLBWT_FM_MATCH=l one lane per query through prim::top_search; the stand-in runs the same functor serially.
    //   The compiler's report for gfx950 (tools/kernel_resources.py; profiles/fm_overlaps/kernel_resources.txt), 32- / 64-bit positions:
    //   k_top_tickets<FmOverlapFn<FmOvCells>> 58 / 58 VGPRs, 8 / 7 waves per SIMD; k_top_tickets<FmOverlapFn<FmOvWalk>> 58 / 62, 8 waves;
    //   k_top_search of the lane forms 40 / 38, 8 waves; prim::k_expand_ranges 18 / 18, 8 waves, 10264 bytes of LDS; no scratch in any of them.
    static constexpr u32 kOverlapProper = 1;
    template <class SRC>
    static void fm_overlaps_run(const FmIndex &F, const FmOverlapFn<SRC> &f, u64 np, OverlapInfo &oi) {
#ifdef GRLBWT_PRIM_HIP
        if (prim::sw().fm_match == 'l') {
            prim::top_search(np, FmOverlapLaneFn<SRC>{f}, F.top_entries, "fm.overlap_lanes");
            oi.lanes = np; oi.refills = 0;
        } else {
            DBuf<u64> ctr(2);
            const prim::WalkStats ws = prim::top_tickets(np, f, ctr.p, F.top_entries, "fm.overlaps");
            oi.lanes = ws.lanes; oi.refills = ws.refills;
        }
#else
        prim::for_each(np, WalkSerialFn<FmOverlapFn<SRC>>{f}, "fm.overlaps");
        oi.lanes = np; oi.refills = 0;
#endif
    }
    static void fm_overlap_args(u32 flags, const u64 *lo, const u64 *hi, const char *who) {
        if (flags & ~kOverlapProper) throw prim::Error(-22, std::string(who) + ": unknown flag bits");
        if ((lo == nullptr) != (hi == nullptr)) throw prim::Error(-22, std::string(who) + ": the row outputs are both given or both null");
    }
    // the two passes over np queries whose cells `src` gives; n_hits is set whenever the count was reached, also when the capacity then refuses the call
    template <class SRC>
    static void fm_overlaps_t(const FmIndex &F, const SRC &src, u64 np, u64 min_len, u64 max_len, u32 flags, u64 *hoff, u64 *olen, u64 *tlo, u64 *thi,
                              u64 *lo, u64 *hi, u64 capacity, u64 &n_hits, const char *who) {
        OverlapInfo oi;
        oi.patterns = np;
        if (np == 0) {
            if (hoff) prim::dev_memset(hoff, 0, 8);
            prim::sync();
            F.oinfo = oi;
            return;
        }
        if (np >= (~0ull >> 4) || (np + 1) * 8 + 64 > prim::mem_available())
            throw prim::Error(-12, std::string(who) + ": the counts need " + std::to_string((np + 1) * 8) + " bytes of device memory, more than is free");
        DBuf<u64> cnt(np + 1);
        DBuf<u32> bad(1);
        bad.zero();
        const u64 floor = min_len ? min_len : 1;
        FmOverlapFn<SRC> f{src, F.key.p, F.slf.p, F.R, F.n, F.sep, floor, max_len ? max_len : ~0ull, (flags & kOverlapProper) != 0,
                           cnt.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bad.p};
        fm_overlaps_run(F, f, np, oi);
        oi.hits = n_hits = prim::reduce_sum<u64>(np, CellIn<u64>{cnt.p}, "fm.overlap_hits");
        if (n_hits > capacity) throw prim::Error(-22, std::string(who) + ": " + std::to_string(n_hits) + " hits, more than the output arrays hold");
        if (!hoff || (n_hits && (!olen || !tlo || !thi))) throw prim::Error(-22, std::string(who) + ": no output arrays");      // (the sizing call takes none)
        prim::exclusive_scan<u64>(np, CellIn<u64>{cnt.p}, hoff, true, "fm.overlap_offsets");
        // (without a hit the arrays may be missing: the pass then stores no entry, and the spare scratch word marks it as the emit pass)
        f.hoff = hoff; f.olen = olen ? olen : cnt.p + np; f.tlo = tlo; f.thi = thi; f.lo = lo; f.hi = hi;
        fm_overlaps_run(F, f, np, oi);
        if (bad.get(0)) throw prim::Error(-71, std::string(who) + ": a query's second pass found another number of hits than its first");
        oi.cells = prim::reduce_sum<u64>(np, FmOvQueryStepsIn{cnt.p}, "fm.overlap_cells");
        oi.steps = oi.cells + prim::reduce_sum<u64>(np, FmOvSepStepsIn{cnt.p, floor}, "fm.overlap_steps");
        if (n_hits) {
            oi.targets = prim::reduce_sum<u64>(n_hits, FmOvSpanIn{tlo, thi}, "fm.overlap_targets");
            oi.longest = prim::reduce_max<u64>(n_hits, CellIn<u64>{olen}, "fm.overlap_longest");
        }
        prim::sync();
        F.oinfo = oi;
    }
    static void fm_overlaps(const FmIndex &F, const void *cells, int w, const u64 *off, u64 np, u64 min_len, u64 max_len, u32 flags, u64 *hoff, u64 *olen,
                            u64 *tlo, u64 *thi, u64 *lo, u64 *hi, u64 capacity, u64 &n_hits) {
        n_hits = 0;
        fm_overlap_args(flags, lo, hi, "fm overlaps");
        u64 x0;
        (void)fm_match_cells(cells, w, off, np, x0, "fm overlaps");
        fm_overlaps_t(F, FmOvCells{fm_count_fn(F, cells, w, off, nullptr, nullptr), F.sepval}, np, min_len, max_len, flags, hoff, olen, tlo, thi, lo, hi,
                      capacity, n_hits, "fm overlaps");
    }
    static void fm_overlaps_of(const FmIndex &F, const u64 *ids, u64 n_ids, u64 min_len, u64 max_len, u32 flags, u64 *hoff, u64 *olen, u64 *tlo, u64 *thi,
                               u64 *lo, u64 *hi, u64 capacity, u64 &n_hits) {
        n_hits = 0;
        fm_overlap_args(flags, lo, hi, "fm overlaps of");
        if (!F.locate) throw prim::Error(-22, "fm overlaps of: the index was made without the structures for locating");
        if (n_ids) {
            const u64 bad = prim::reduce_min<u64>(n_ids, FmOvIdBadIn{ids, F.k}, "fm.overlap_ids");
            if (bad != ~0ull) throw prim::Error(-22, "fm overlaps of: entry " + std::to_string(bad) + " is not below the number of strings");
        }
        fm_overlaps_t(F, FmOvWalk{F.lf(), F.sep, ids}, n_ids, min_len, max_len, flags, hoff, olen, tlo, thi, lo, hi, capacity, n_hits, "fm overlaps of");
    }
    // prefix ranks -> string numbers: sid[t] for every t of every range, back to back.  The device form is prim::expand_ranges (one
    // tile of kOverlapTile entries per workgroup); the stand-in's, and the form it is measured against, a for_each over the entries
    // with a search in the scanned offsets.  n_entries is set whenever the count was reached, also when the capacity then refuses the call.
    static void fm_overlap_targets(const FmIndex &F, const u64 *tlo, const u64 *thi, u64 nr, u64 *eoff, u64 *str, u64 *rng, u64 capacity, u64 &n_entries) {
        n_entries = 0;
        if (!F.locate) throw prim::Error(-22, "fm overlap targets: the index was made without the structures for locating");
        OverlapInfo oi;
        oi.ranges = nr;
        if (nr == 0) {
            if (eoff) prim::dev_memset(eoff, 0, 8);
            prim::sync();
            F.oinfo = oi;
            return;
        }
        const u64 bad = prim::reduce_min<u64>(nr, FmOvRangeBadIn{tlo, thi, F.k}, "fm.overlap_ranges");
        if (bad != ~0ull) throw prim::Error(-22, "fm overlap targets: range " + std::to_string(bad) + " is no range of prefix ranks (lo <= hi <= the number of strings)");
        if (nr >= ((u64)1 << 32)) throw prim::Error(-75, "fm overlap targets: more ranges than one call takes");
        if ((nr + 1) * 8 + 64 > prim::mem_available())
            throw prim::Error(-12, "fm overlap targets: the offsets need " + std::to_string((nr + 1) * 8) + " bytes of device memory, more than is free");
        DBuf<u64> sc(nr + 1);
        oi.entries = n_entries = prim::exclusive_scan<u64>(nr, FmOvSpanIn{tlo, thi}, sc.p, true, "fm.overlap_entry_offsets");
        if (n_entries > capacity) throw prim::Error(-22, "fm overlap targets: " + std::to_string(n_entries) + " entries, more than the output arrays hold");
        if (!eoff || (n_entries && !str)) throw prim::Error(-22, "fm overlap targets: no output arrays");      // (the sizing call takes none)
        prim::d2d(eoff, sc.p, (nr + 1) * 8);
        if (n_entries) {
#ifdef GRLBWT_PRIM_HIP
            if (prim::sw().dev_overlap_expand != 'f') prim::expand_ranges<idx_t>(nr, n_entries, sc.p, tlo, F.sid.p, str, rng, "fm.overlap_expand");
            else
#endif
                prim::for_each(n_entries, FmOvExpandFn{sc.p, tlo, F.sid.p, nr, str, rng}, "fm.overlap_expand_plain");
        }
        prim::sync();
        F.oinfo = oi;
    }
    // ---- the LCP array and the suffix-length counts (functor block "the LCP array of the collection").  Everything
    // that can refuse the call for its arguments or for memory runs before the first store into an output; histograms that may
    // not fit their capacity are sized by a run that stores nothing.  Scratch, about 0.9 byte per row: two generations of B and
    // of S, the ranks of B, the F-order run-start bit-vector with its RankCells (and a word per tile of the fused pass).
    //   A pass in its generic form goes through the primitives alone (the serial stand-in's form, and with GRLBWT_LCP_ROUND=p the
    //   device's): ranks of B (scan), B' and S' (bitvector_from_pred), B' & ~B and its ranks, the values (for_each_set_bit), |S'|
    //   (reduce_sum).  The device form is prim::LcpRound: one kernel that writes B', S' and the values and counts per tile.
    //   Loops: at most cap - 1 passes, each of which sets a bit or ends the call; nothing waits for another thread, and a pass has no atomics.
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kLcpTile = prim::kLcpTile;
#else
    static constexpr u64 kLcpTile = 4096;        // (the serial form has no tiles: the figure the device library reports)
#endif
    // one bit per slf[j], the first row of every sorted run, with ranks: run_of_row over F order (the forward step's lookup)
    static void fm_run_cells(const FmIndex &F, DBuf<RankCell> &frc) {
        RankBits rb;
        build_rankbits(rb, F.slf.p, F.R, F.n + 1, "lcp.runbits");
        const u64 nc = (F.n + 1) / 64 + 2;
        frc.alloc(nc);
        prim::for_each(nc, RankCellFn{rb.words.p, rb.base.p, frc.p}, "lcp.rankcells");
    }
    struct FmLcp {
        u64 n = 0, nw = 0;
        bool plain = !prim::kIsDevice;
        DBuf<RankCell> frc;
        DBuf<u64> b0, b1, s0, s1;
        DBuf<idx_t> brank;
        static u64 words_of(u64 n_) { return n_ / 64 + 2; }
        static u64 tiles_of(u64 n_) { return (n_ + kLcpTile - 1) / kLcpTile; }
        static u64 scratch_bytes(u64 n_) {
            return 4 * words_of(n_) * 8 + (words_of(n_) + 1) * sizeof(idx_t) + ((n_ + 1) / 64 + 2) * sizeof(RankCell) + tiles_of(n_) * 8;
        }
#ifdef GRLBWT_PRIM_HIP
        prim::LcpRound W;
#endif
        void alloc(const FmIndex &F) {
            n = F.n; nw = words_of(n);
#ifdef GRLBWT_PRIM_HIP
            plain = prim::sw().lcp_round == 'p';
            if (!plain) W.alloc(n);
#endif
            fm_run_cells(F, frc);
            b0.alloc(nw); b1.alloc(nw); s0.alloc(nw); s1.alloc(nw); brank.alloc(nw + 1);
        }
        LcpRowFn rows(const FmIndex &F, const u64 *B, const u64 *S) const { return LcpRowFn{frc.p, F.key.p, F.slf.p, F.k, B, brank.p, S}; }
        // B (with its ranks in brank) and S -> Bn and Sn; v at the newly set rows of out (null: no store).  B is used up.
        void pass_plain(const LcpRowFn &f, u64 *B, u64 *Bn, u64 *Sn, void *out, int w, u64 v, u64 &n_new, u64 &n_suf) {
            prim::bitvector_from_pred(n, LcpPassPred{f}, Bn, "lcp.bits");
            prim::bitvector_from_pred(n, LcpLenPred{f}, Sn, "lcp.lengths");
            prim::for_each((n + 63) / 64, LcpNewFn{Bn, B}, "lcp.new");
            n_new = (u64)prim::exclusive_scan<idx_t>(nw, PopcIn{B}, brank.p, true, "lcp.new_ranks");
            if (out && n_new) prim::for_each_set_bit<idx_t>(n, B, brank.p, LcpStoreFn{out, w, v}, "lcp.values");
            n_suf = prim::reduce_sum<u64>((n + 63) / 64, PopcIn{Sn}, "lcp.suffixes");
        }
        // (acc, for fm_kmers: a bit-vector that every generation of S is OR-ed into; the last generations stay in Bfin / Sfin,
        // the used-up ones in Bold / Sold)
        u64 *Bfin = nullptr, *Sfin = nullptr, *Bold = nullptr, *Sold = nullptr;
        void run(const FmIndex &F, u64 cap, void *out, int w, LcpInfo &li, std::vector<u64> &rows_at, std::vector<u64> &suf, u64 *acc = nullptr) {
            rows_at.clear(); suf.clear();
            b0.zero(); b1.zero(); s0.zero(); s1.zero();
            u64 *B = b0.p, *Bn = b1.p, *S = s0.p, *Sn = s1.p;
            prim::bitvector_from_pred(n, LcpHeadPred{rows(F, nullptr, nullptr)}, B, "lcp.heads");
            prim::bitvector_from_pred(n, LcpBelowPred{F.k}, S, "lcp.terminators");
            if (out) prim::dev_memset(out, 0, n * (u64)w);
            u64 set = prim::reduce_sum<u64>((n + 63) / 64, PopcIn{B}, "lcp.heads_sum");
            rows_at.push_back(set); suf.push_back(F.k);
            u64 passes = 0;
            while (set < n && passes + 1 < cap) {
                const u64 v = passes + 1;
                u64 n_new = 0, n_suf = 0;
                const LcpRowFn f = rows(F, B, S);
#ifdef GRLBWT_PRIM_HIP
                if (!plain) {
                    prim::exclusive_scan_nosync<idx_t>(nw, PopcIn{B}, brank.p, true, "lcp.ranks");
                    W.pass(f, B, Bn, Sn, out, w, v, &n_new, &n_suf);
                } else
#endif
                {
                    (void)prim::exclusive_scan<idx_t>(nw, PopcIn{B}, brank.p, true, "lcp.ranks");
                    pass_plain(f, B, Bn, Sn, out, w, v, n_new, n_suf);
                }
                if (n_new == 0)
                    throw prim::Error(-22, "fm lcp: pass " + std::to_string(v) + " set no row while " + std::to_string(n - set) +
                                               " rows are open: not the BWT of a collection");
                rows_at.push_back(n_new); suf.push_back(n_suf);
                set += n_new; passes++;
                std::swap(B, Bn); std::swap(S, Sn);
                if (acc) prim::for_each((n + 63) / 64, KmerOrFn{S, acc}, "lcp.lengths_or");
            }
            Bfin = B; Sfin = S; Bold = Bn; Sold = Sn;
            li.passes = passes; li.n_levels = passes + 1; li.n_capped = n - set;
            li.max_lcp = li.n_capped ? cap : passes;
            if (out && li.n_capped) {     // the rows still open: their LCP is cap or more
                prim::bitvector_from_pred(n, LcpUnsetPred{B}, Bn, "lcp.open");
                (void)prim::exclusive_scan<idx_t>(nw, PopcIn{Bn}, brank.p, true, "lcp.open_ranks");
                prim::for_each_set_bit<idx_t>(n, Bn, brank.p, LcpStoreFn{out, w, cap}, "lcp.capped");
            }
        }
    };
    // n_levels is set whenever the passes were run, also when the capacity then refuses the call
    static void fm_lcp(const FmIndex &F, u64 max_lcp, int w, void *out, u64 *rows_at, u64 *suffixes_of, u64 hist_capacity, u64 &n_levels) {
        n_levels = 0;
        if (!(w == 1 || w == 2 || w == 4 || w == 8)) throw prim::Error(-22, "fm lcp: the values take 1, 2, 4 or 8 bytes");
        if (!out && !rows_at && !suffixes_of) throw prim::Error(-22, "fm lcp: no output");
        const u64 lim = w == 8 ? ~0ull : (1ull << (8 * w)) - 1;
        const u64 cap = max_lcp && max_lcp < lim ? max_lcp : lim;
        const bool hist = rows_at || suffixes_of;
        LcpInfo li;
        li.n = F.n; li.k = F.k; li.lcp_bytes = (u64)w; li.cap = cap; li.tile_rows = kLcpTile;
        std::vector<u64> ra(1, 0), su(1, 0);
        if (F.n) {
            li.scratch_bytes = FmLcp::scratch_bytes(F.n);
            if (F.n >= ((u64)1 << 62) || li.scratch_bytes > prim::mem_available())
                throw prim::Error(-12, "fm lcp: the passes need " + std::to_string(li.scratch_bytes) + " bytes of device memory, more than is free");
            FmLcp L;
            L.alloc(F);
            // at most cap levels, and a pass sets a row: where the histograms may not hold them, a run without stores sizes them
            const u64 bound = cap < F.n + 1 ? cap : F.n + 1;
            const bool sizing = out && hist && hist_capacity < bound;
            if (sizing) L.run(F, cap, nullptr, w, li, ra, su);
            if (!sizing || li.n_levels <= hist_capacity) L.run(F, cap, out, w, li, ra, su);
        } else {
            li.n_levels = 1;
        }
        prim::sync();
        F.linfo = li;
        n_levels = li.n_levels;
        if (hist && n_levels > hist_capacity)
            throw prim::Error(-22, "fm lcp: " + std::to_string(n_levels) + " levels, more than the histograms hold");
        if (rows_at) std::memcpy(rows_at, ra.data(), n_levels * 8);
        if (suffixes_of) std::memcpy(suffixes_of, su.data(), n_levels * 8);
    }
    // what grlbwt_fm_kmers and grlbwt_debruijn_create share: the LCP passes capped at k and the length passes (B: the rows with
    // LCP < k; H: the heads), the non-empty words of B for KmerCountFn, and the selection with its ranks (in L.brank)
    struct KmerSel {
        FmLcp L;
        DBuf<u64> NZ;
        DBuf<idx_t> nzbase, nzlist;
        const u64 *B = nullptr;
        u64 *H = nullptr, *sel = nullptr;
        u64 n = 0, nnz = 0;
        KmerCountFn cnt() const { return KmerCountFn{B, NZ.p, nzbase.p, nzlist.p, nnz, n}; }
        static u64 scratch_bytes(u64 n_) {
            const u64 nw = FmLcp::words_of(n_), nwords = (n_ + 63) / 64, nzw = nwords / 64 + 2;
            return FmLcp::scratch_bytes(n_) + nw * 8 + nzw * 8 + (nzw + 1 + nwords) * sizeof(idx_t);
        }
        void heads(const FmIndex &F, u64 k, KmerInfo &ki) {
            n = F.n;
            const u64 nw = FmLcp::words_of(n), nwords = (n + 63) / 64, nzw = nwords / 64 + 2;
            L.alloc(F);
            DBuf<u64> sh(nw);
            sh.zero();
            prim::bitvector_from_pred(n, LcpBelowPred{F.k}, sh.p, "kmer.terminators");
            LcpInfo li;
            std::vector<u64> ra, su;
            L.run(F, k, nullptr, 8, li, ra, su, sh.p);               // B: the rows with LCP < k
            ki.passes = li.passes;
            {   // the suffixes of passes + 1 .. k - 1 cells: copy-only passes of S, until a generation is empty
                u64 *S = L.Sfin, *Sn = L.Sold, last = su.back();
                for (u64 l = li.passes + 1; l < k && last; l++) {
                    prim::bitvector_from_pred(n, LcpLenPred{L.rows(F, nullptr, S)}, Sn, "kmer.lengths");
                    last = prim::reduce_sum<u64>(nwords, PopcIn{Sn}, "kmer.suffixes");
                    prim::for_each(nwords, KmerOrFn{Sn, sh.p}, "kmer.lengths_or");
                    std::swap(S, Sn);
                    ki.length_passes++;
                }
            }
            B = L.Bfin; H = L.Bold; sel = L.Sfin;
            prim::for_each(nwords, KmerHeadsFn{B, sh.p, H}, "kmer.heads");
            sh.release();
            NZ.alloc(nzw); nzbase.alloc(nzw + 1);
            NZ.zero();
            prim::bitvector_from_pred(nwords, KmerWordPred{B}, NZ.p, "kmer.words");
            nnz = (u64)prim::exclusive_scan<idx_t>(nzw, PopcIn{NZ.p}, nzbase.p, true, "kmer.word_ranks");
            nzlist.alloc(nnz);
            prim::for_each_set_bit<idx_t>(nwords, NZ.p, nzbase.p, KmerWordListFn{nzlist.p}, "kmer.word_list");
        }
        void select(const KmerFilter &flt, KmerInfo &ki) {
            const u64 nw = FmLcp::words_of(n);
            prim::dev_memset(sel, 0, nw * 8);
            prim::bitvector_from_pred(n, KmerSelPred{H, cnt(), flt}, sel, "kmer.select");
            ki.n_selected = (u64)prim::exclusive_scan<idx_t>(nw, PopcIn{sel}, L.brank.p, true, "kmer.select_ranks");
        }
        // the same over the representatives of the strand-merged classes, by total (fm_ckmers); returns the number selected
        u64 select_classes(const u64 *rep, const CkTotalFn &tot, const KmerFilter &flt) {
            const u64 nw = FmLcp::words_of(n);
            prim::dev_memset(sel, 0, nw * 8);
            prim::bitvector_from_pred(n, CkSelPred{rep, tot, flt}, sel, "ckmer.select");
            return (u64)prim::exclusive_scan<idx_t>(nw, PopcIn{sel}, L.brank.p, true, "ckmer.select_ranks");
        }
    };
    // ---- the distinct k-mers with their counts (functor block "the distinct k-mers with their counts").  Everything
    // that can refuse the call runs before the first store: the arguments, the memory, the passes (an image that is not the BWT
    // of a collection), the capacity.  Then the spectrum is copied to the host and the table is decoded.
    //   Loops: at most k - 1 LCP passes, each of which sets a row or ends the call; at most k - 1 length passes, which end with the
    //   first generation of S that is empty (no string has that many cells, so none has more); a head's count takes no loop
    //   (KmerCountFn); the decode takes k steps per entry.  Nothing waits for another thread; the only atomics are the
    //   histogram's (LDS, and one per used bin and workgroup at the flush).
    static void fm_kmers(const FmIndex &F, u64 k, u64 min_count, u64 max_count, u64 row_begin, u64 row_end, int w, void *cells, u64 *lo, u64 *count,
                         u64 capacity, u64 &n_kmers, bool want_n, u64 *host_spectrum, u64 bins) {
        n_kmers = 0;
        if (k == 0) throw prim::Error(-22, "fm kmers: k is 0");
        if (!(w == 1 || w == 2 || w == 4 || w == 8)) throw prim::Error(-22, "fm kmers: cell_bytes is " + std::to_string(w) + ", not 1, 2, 4 or 8");
        if (!cells && !lo && !count && !host_spectrum && !want_n) throw prim::Error(-22, "fm kmers: no output");
        if (host_spectrum && (bins == 0 || bins > kKmerMaxBins))
            throw prim::Error(-22, "fm kmers: " + std::to_string(bins) + " spectrum bins, not 1 to " + std::to_string(kKmerMaxBins));
        const u64 n = F.n;
        if (row_end > n) row_end = n;                            // (UINT64_MAX: n_rows)
        if (row_begin > row_end)
            throw prim::Error(-22, "fm kmers: rows [" + std::to_string(row_begin) + ", " + std::to_string(row_end) + ") are no window of " + std::to_string(n) + " rows");
        if (cells && w < 8 && F.R) {
            const u64 top = F.alpha.p ? F.alpha.get(F.alpha.n - 1) : (u64)F.key.get(F.R - 1).host_sym();
            if (top >> (8 * w)) throw prim::Error(-22, "fm kmers: the image's largest symbol " + std::to_string(top) + " does not fit cell_bytes = " + std::to_string(w));
        }
        if ((cells && ((uintptr_t)cells & (uintptr_t)(w - 1))) || ((uintptr_t)lo & 7) || ((uintptr_t)count & 7))
            throw prim::Error(-22, "fm kmers: an output is not aligned to its width");
        const bool table = cells || lo || count;
        const u64 nb = host_spectrum ? bins : 1;
        KmerInfo ki;
        ki.k = k; ki.n = n; ki.n_strings = F.k;
        std::vector<u64> spec(nb, 0);
        if (n == 0) { F.kinfo = ki; if (host_spectrum) std::memcpy(host_spectrum, spec.data(), nb * 8); return; }
        const u64 nw = FmLcp::words_of(n), nwords = (n + 63) / 64, nzw = nwords / 64 + 2;
        ki.scratch_bytes = FmLcp::scratch_bytes(n) + nw * 8 + nzw * 8 + (nzw + 1 + nwords) * sizeof(idx_t) + nb * 8;
        if (n >= ((u64)1 << 62) || ki.scratch_bytes > prim::mem_available())
            throw prim::Error(-12, "fm kmers: the passes need " + std::to_string(ki.scratch_bytes) + " bytes of device memory, more than is free");
        KmerSel K;
        K.heads(F, k, ki);
        FmLcp &L = K.L;
        const u64 *H = K.H;
        u64 *sel = K.sel;
        const KmerCountFn cnt = K.cnt();
        DBuf<u64> dbins(nb);
#ifdef GRLBWT_PRIM_HIP
        prim::kmer_spectrum(n, H, cnt, (u32)nb, dbins.p, ki.n_distinct, ki.n_windows, ki.largest_count);
#else
        dbins.zero();
        (void)prim::exclusive_scan<idx_t>(nw, PopcIn{H}, L.brank.p, true, "kmer.head_ranks");
        prim::for_each_set_bit<idx_t>(n, H, L.brank.p, KmerSpectrumFn{cnt, dbins.p, nb - 1}, "kmer.spectrum");
        ki.n_distinct = prim::reduce_sum<u64>(nwords, PopcIn{H}, "kmer.heads_sum");
        ki.n_windows = prim::reduce_sum<u64>(n, KmerWindowsIn{H, cnt}, "kmer.windows");
        ki.largest_count = prim::reduce_max<u64>(n, KmerWindowsIn{H, cnt}, "kmer.largest");
#endif
        prim::d2h(spec.data(), dbins.p, nb * 8);
        const KmerFilter flt{row_begin, row_end, min_count ? min_count : 1, max_count ? max_count : ~0ull};
        K.select(flt, ki);
        ki.forward_steps = cells ? ki.n_selected * k : 0;
        prim::sync();
        F.kinfo = ki;
        n_kmers = ki.n_selected;
        if (table && n_kmers > capacity)
            throw prim::Error(-22, "fm kmers: " + std::to_string(n_kmers) + " k-mers, more than the output arrays hold");
        if (host_spectrum) std::memcpy(host_spectrum, spec.data(), nb * 8);
        if (!table || n_kmers == 0) return;
        const KmerStepFn step{L.frc.p, F.key.p, F.slf.p, F.alpha.p};
        with_cell(w, [&](auto c) {
            typedef decltype(c) cell_t;
#ifdef GRLBWT_PRIM_HIP
            if (prim::sw().dev_kmer_decode != 'f') prim::kmer_decode<cell_t, idx_t>(n_kmers, k, sel, L.brank.p, n, step, cnt, (cell_t *)cells, lo, count);
            else
#endif
                prim::for_each_set_bit<idx_t>(n, sel, L.brank.p, KmerEmitFn<cell_t>{step, cnt, k, (cell_t *)cells, lo, count}, "kmer.decode_plain");
        });
        prim::sync();
    }
    // what grlbwt_fm_kmers_canonical and grlbwt_cdebruijn_create share, as KmerSel is shared below them: the checks of the complement
    // map, its table of (code, comp code), the passes, the head ranks, the mate pass with its counters and the representatives'
    // bits (in L.Sold).  The caller keeps the order of events: pairs(), its own refusals for memory, table(), heads(), mates().
    struct CkSel {
        KmerSel K;
        std::vector<u64> vals;        // the pairs' values, 2 * n_pairs
        std::vector<u32> codes;       // and their symbol codes (kCkAbsent: not in the image)
        u64 n_pairs = 0;
        DBuf<CkPair> dtab;
        DBuf<idx_t> hrank, mate;
        u32 nt = 0;
        bool rest = false;
        u64 n_distinct = 0, backward_steps = 0, forward_steps = 0, mate_walks = 0;
        u64 fixed_bytes() const { return kCkMaxTable * sizeof(CkPair) + 2 * n_pairs * 12 + (kCkStripes * 4 + 2) * 8; }
        // every value in at most one pair, the separator in none
        void pairs(const char *kWho, const FmIndex &F, const u64 *host_pairs, u64 np) {
            if (np > 128) throw prim::Error(-22, std::string(kWho) + "n_pairs is " + std::to_string(np) + ", more than 128");
            if (!host_pairs && np) throw prim::Error(-22, std::string(kWho) + "host_pairs is NULL with n_pairs = " + std::to_string(np));
            static const u64 kDna[4] = {'A', 'T', 'C', 'G'};
            if (!host_pairs) { host_pairs = kDna; np = 2; }
            n_pairs = np;
            vals.assign(host_pairs, host_pairs + 2 * np);
            std::vector<u64> seen;
            for (u64 i = 0; i < np; i++) {
                seen.push_back(vals[2 * i]);
                if (vals[2 * i + 1] != vals[2 * i]) seen.push_back(vals[2 * i + 1]);
            }
            std::sort(seen.begin(), seen.end());
            for (size_t i = 1; i < seen.size(); i++)
                if (seen[i] == seen[i - 1]) throw prim::Error(-22, std::string(kWho) + "the value " + std::to_string(seen[i]) + " is listed twice in the pairs");
            if (F.R && std::binary_search(seen.begin(), seen.end(), F.sepval))
                throw prim::Error(-22, std::string(kWho) + "the separator's value " + std::to_string(F.sepval) + " is in a pair");
        }
        // the table of (code, comp code), in ascending code: the values go to codes on the device
        void table(const FmIndex &F) {
            dtab.alloc(kCkMaxTable);
            nt = 0;
            if (n_pairs) {
                DBuf<u64> dv(2 * n_pairs);
                DBuf<u32> dc(2 * n_pairs);
                prim::h2d(dv.p, vals.data(), 2 * n_pairs * 8);
                prim::for_each(2 * n_pairs, CkCodeFn{fm_count_fn(F, nullptr, 8, nullptr, nullptr, nullptr), dv.p, dc.p}, "ckmer.codes");
                codes = dc.to_host(2 * n_pairs);
                std::vector<CkPair> tab;
                for (u64 i = 0; i < n_pairs; i++) {
                    const u32 a = codes[2 * i], b = codes[2 * i + 1];
                    if (a != kCkAbsent) tab.push_back(CkPair{a, b});
                    if (b != kCkAbsent && vals[2 * i] != vals[2 * i + 1]) tab.push_back(CkPair{b, a});
                }
                std::sort(tab.begin(), tab.end(), [](const CkPair &x, const CkPair &y) { return x.code < y.code; });
                nt = (u32)tab.size();
                if (nt) prim::h2d(dtab.p, tab.data(), nt * sizeof(CkPair));
            }
            rest = (u64)nt + 1 < F.sigma;                        // a symbol besides the separator has no pair
        }
        void heads(const FmIndex &F, u64 k, KmerInfo &ki) {
            K.heads(F, k, ki);
            const u64 nw = FmLcp::words_of(F.n);
            hrank.alloc(nw + 1);
            n_distinct = (u64)prim::exclusive_scan<idx_t>(nw, PopcIn{K.H}, hrank.p, true, "ckmer.head_ranks");
        }
        void mates(const char *kWho, const FmIndex &F, u64 k) {
            const u64 n = F.n;
            if (n_distinct * sizeof(idx_t) > prim::mem_available())
                throw prim::Error(-12, std::string(kWho) + "the mates need " + std::to_string(n_distinct * sizeof(idx_t)) + " bytes of device memory, more than is free");
            mate.alloc(n_distinct);
            mate.fill_ff();
            if (!n_distinct) return;
            DBuf<u64> ctr(kCkStripes * 4 + 2);
            ctr.zero();
            const KmerMateFn f{K.L.frc.p, F.key.p, F.slf.p, F.R, n, k < n ? k : n, K.H, K.cnt(), dtab.p, nt, rest, mate.p, ctr.p};
#ifdef GRLBWT_PRIM_HIP
            if (prim::sw().dev_kmer_mates != 'f') (void)prim::kmer_mates<idx_t>(n_distinct, f, K.H, hrank.p, n, ctr.p + kCkStripes * 4, F.top_entries);
            else
#endif
                prim::for_each_set_bit<idx_t>(n, K.H, hrank.p, KmerMateEachFn{f}, "ckmer.mates_plain");
            const std::vector<u64> hc = ctr.to_host(kCkStripes * 4);
            u64 idle = 0;
            for (u64 s = 0; s < kCkStripes; s++) { backward_steps += hc[4 * s]; forward_steps += hc[4 * s + 1]; idle += hc[4 * s + 2]; }
            mate_walks = n_distinct - idle;
        }
        const u64 *representatives() {
            u64 *rep = K.L.Sold;
            prim::dev_memset(rep, 0, FmLcp::words_of(K.n) * 8);
            prim::bitvector_from_pred(K.n, CkRepPred{CkRank{K.H, hrank.p}, mate.p}, rep, "ckmer.representatives");
            return rep;
        }
    };
    // ---- the strand-merged k-mers (functor block "the strand-merged k-mers").  fm_kmers' order of events: the
    // arguments and the complement map, the memory, the passes, the mates (whose array is sized by the head count), the capacity;
    // then the spectrum is copied to the host and the table is written.  Nothing is stored into an output before the last refusal.
    //   Device form of the mate pass: prim::kmer_mates, one ticket per head rank under the LDS top level with the complement
    //   table in LDS; generic form, the serial stand-in's and with GRLBWT_DEV_KMER_MATES=f the device's: for_each_set_bit over H.
    //   The cells, lo and count go through fm_kmers' own decode; mate_lo and total through one for_each_set_bit over the selection.
    //   Loops: those of fm_kmers, and at most min(k, n) steps per head in the mate pass.  Nothing waits for another thread.
    static void fm_ckmers(const FmIndex &F, u64 k, u64 min_count, u64 max_count, u64 row_begin, u64 row_end, const u64 *host_pairs, u64 n_pairs, int w,
                          void *cells, u64 *lo, u64 *count, u64 *mate_lo, u64 *total, u64 capacity, u64 &n_classes, bool want_n, u64 *host_spectrum,
                          u64 bins) {
        static const char *const kWho = "fm canonical kmers: ";
        n_classes = 0;
        if (k == 0) throw prim::Error(-22, std::string(kWho) + "k is 0");
        if (!(w == 1 || w == 2 || w == 4 || w == 8)) throw prim::Error(-22, std::string(kWho) + "cell_bytes is " + std::to_string(w) + ", not 1, 2, 4 or 8");
        if (!cells && !lo && !count && !mate_lo && !total && !host_spectrum && !want_n) throw prim::Error(-22, std::string(kWho) + "no output");
        if (host_spectrum && (bins == 0 || bins > kKmerMaxBins))
            throw prim::Error(-22, std::string(kWho) + std::to_string(bins) + " spectrum bins, not 1 to " + std::to_string(kKmerMaxBins));
        const u64 n = F.n;
        if (row_end > n) row_end = n;                            // (UINT64_MAX: n_rows)
        if (row_begin > row_end)
            throw prim::Error(-22, std::string(kWho) + "rows [" + std::to_string(row_begin) + ", " + std::to_string(row_end) + ") are no window of " +
                                       std::to_string(n) + " rows");
        if (cells && w < 8 && F.R) {
            const u64 top = F.alpha.p ? F.alpha.get(F.alpha.n - 1) : (u64)F.key.get(F.R - 1).host_sym();
            if (top >> (8 * w))
                throw prim::Error(-22, std::string(kWho) + "the image's largest symbol " + std::to_string(top) + " does not fit cell_bytes = " + std::to_string(w));
        }
        if ((cells && ((uintptr_t)cells & (uintptr_t)(w - 1))) || ((uintptr_t)lo & 7) || ((uintptr_t)count & 7) || ((uintptr_t)mate_lo & 7) || ((uintptr_t)total & 7))
            throw prim::Error(-22, std::string(kWho) + "an output is not aligned to its width");
        CkSel S;
        S.pairs(kWho, F, host_pairs, n_pairs);
        const bool table = cells || lo || count || mate_lo || total;
        const u64 nb = host_spectrum ? bins : 1;
        CkmerInfo ci;
        ci.k = k; ci.n = n; ci.n_strings = F.k;
        std::vector<u64> spec(nb, 0);
        if (n == 0) { F.cinfo = ci; if (host_spectrum) std::memcpy(host_spectrum, spec.data(), nb * 8); return; }
        const u64 nw = FmLcp::words_of(n);
        const u64 fixed = S.fixed_bytes();
        ci.scratch_bytes = KmerSel::scratch_bytes(n) + nb * 8 + (nw + 1) * sizeof(idx_t) + fixed;
        if (n >= ((u64)1 << 62) || ci.scratch_bytes > prim::mem_available())
            throw prim::Error(-12, std::string(kWho) + "the passes need " + std::to_string(ci.scratch_bytes) + " bytes of device memory, more than is free");
        S.table(F);
        KmerSel &K = S.K;
        KmerInfo ki;
        S.heads(F, k, ki);
        ci.passes = ki.passes; ci.length_passes = ki.length_passes;
        FmLcp &L = K.L;
        const u64 *H = K.H;
        const KmerCountFn cnt = K.cnt();
        ci.n_distinct = S.n_distinct;
        ci.scratch_bytes += ci.n_distinct * sizeof(idx_t);
        S.mates(kWho, F, k);
        ci.backward_steps = S.backward_steps; ci.forward_steps = S.forward_steps; ci.mate_walks = S.mate_walks;
        const DBuf<idx_t> &hrank = S.hrank, &mate = S.mate;
        // ---- representatives, totals, the spectrum, the classes
        const CkRank rk{H, hrank.p};
        const CkTotalFn tot{cnt, rk, mate.p};
        const u64 *rep = S.representatives();
        DBuf<u64> dbins(nb);
#ifdef GRLBWT_PRIM_HIP
        prim::kmer_spectrum(n, rep, tot, (u32)nb, dbins.p, ci.n_classes, ci.n_windows, ci.largest_total);
#else
        dbins.zero();
        (void)prim::exclusive_scan<idx_t>(nw, PopcIn{rep}, L.brank.p, true, "ckmer.class_ranks");
        prim::for_each_set_bit<idx_t>(n, rep, L.brank.p, CkSpectrumFn{tot, dbins.p, nb - 1}, "ckmer.spectrum");
        ci.n_classes = prim::reduce_sum<u64>((n + 63) / 64, PopcIn{rep}, "ckmer.classes");
        ci.n_windows = prim::reduce_sum<u64>(n, CkWindowsIn{rep, tot}, "ckmer.windows");
        ci.largest_total = prim::reduce_max<u64>(n, CkWindowsIn{rep, tot}, "ckmer.largest");
#endif
        prim::d2h(spec.data(), dbins.p, nb * 8);
        ci.n_paired = prim::reduce_sum<u64>(n, CkClassIn{rk, mate.p, 0}, "ckmer.paired");
        ci.n_palindromes = prim::reduce_sum<u64>(n, CkClassIn{rk, mate.p, 1}, "ckmer.palindromes");
        ci.n_no_complement = prim::reduce_sum<u64>(n, CkClassIn{rk, mate.p, 2}, "ckmer.no_complement");
        ci.n_single = ci.n_classes - ci.n_paired - ci.n_palindromes;
        const KmerFilter flt{row_begin, row_end, min_count ? min_count : 1, max_count ? max_count : ~0ull};
        ci.n_selected = K.select_classes(rep, tot, flt);
        if (cells) ci.forward_steps += ci.n_selected * k;
        prim::sync();
        F.cinfo = ci;
        n_classes = ci.n_selected;
        if (table && n_classes > capacity)
            throw prim::Error(-22, std::string(kWho) + std::to_string(n_classes) + " classes, more than the output arrays hold");
        if (host_spectrum) std::memcpy(host_spectrum, spec.data(), nb * 8);
        if (!table || n_classes == 0) return;
        const u64 *sel = K.sel;
        if (cells || lo || count) {
            const KmerStepFn step{L.frc.p, F.key.p, F.slf.p, F.alpha.p};
            with_cell(w, [&](auto c) {
                typedef decltype(c) cell_t;
#ifdef GRLBWT_PRIM_HIP
                if (prim::sw().dev_kmer_decode != 'f') prim::kmer_decode<cell_t, idx_t>(n_classes, k, sel, L.brank.p, n, step, cnt, (cell_t *)cells, lo, count);
                else
#endif
                    prim::for_each_set_bit<idx_t>(n, sel, L.brank.p, KmerEmitFn<cell_t>{step, cnt, k, (cell_t *)cells, lo, count}, "kmer.decode_plain");
            });
        }
        if (mate_lo || total) prim::for_each_set_bit<idx_t>(n, sel, L.brank.p, CkEmitFn{tot, mate_lo, total}, "ckmer.emit");
        prim::sync();
    }
    // ---- the right-maximal and maximal repeats (functor block "the right-maximal and maximal repeats").  Everything
    // that can refuse the call runs before the first store: the arguments, the memory, the passes (an image that is not the BWT
    // of a collection), the capacity.  Scratch: the LCP passes', the values with their minima (value_bytes * n * 64 / 63), a
    // word of ranks per 64 rows for the run heads; the heads and the selection reuse two bit-vectors of the passes.
    //   Device form: prim::repeat_minima (a wave per node) and prim::repeat_search (a tile of kRepTileRows rows per workgroup, the
    //   tile's values and node minima in LDS; counts and selects in one pass).  Generic form, the serial stand-in's and with
    //   GRLBWT_DEV_REPEAT_SEARCH=f the device's: a for_each per level, four reduces and bitvector_from_pred over functors that
    //   search the tree in memory.  The emit is the same in both: for_each_set_bit over the selected rows, which repeats their
    //   two searches in the tree in memory (no bytes of scratch per row); a tile kernel for it measured slower and is not kept.
    //   Loops: at most cap - 1 LCP passes; the levels (at most 11); a search is bounded (rep_search_back).  Nothing waits for
    //   another thread; the only atomics are the ORs that set the head bits.
    static constexpr u32 kRepMaximal = 1u;
    template <class VT>
    static void fm_repeats_t(const FmIndex &F, FmLcp &L, RepeatInfo &ri, const RepFilter &flt, u64 cap, u64 *lo, u64 *count, u64 *len, u64 *split,
                             u64 capacity, bool table, u64 &n_repeats) {
        const u64 n = F.n, nw = FmLcp::words_of(n);
        const u32 levels = (u32)ri.tree_levels;
        DBuf<VT> tree(rep_entries(n));
        DBuf<idx_t> hrank(nw + 1);
        {
            LcpInfo li;
            std::vector<u64> ra, su;
            L.run(F, cap, tree.p, (int)sizeof(VT), li, ra, su);
            ri.passes = li.passes;
        }
#ifdef GRLBWT_PRIM_HIP
        const bool tiles = prim::sw().dev_repeat_search != 'f';
#endif
        {
            u64 off = 0;
            for (u32 l = 0; l + 1 < levels; l++) {
                const u64 ns = rep_cnt(n, l), nd = rep_cnt(n, l + 1);
#ifdef GRLBWT_PRIM_HIP
                if (tiles) prim::repeat_minima<VT>(tree.p + off, ns, tree.p + off + ns, nd);
                else
#endif
                    prim::for_each(nd, RepMinFn<VT>{tree.p + off, ns, tree.p + off + ns}, "repeat.minima_plain");
                off += ns;
            }
        }
        u64 *hb = L.Bold, *sel = L.Sold;
        prim::dev_memset(hb, 0, nw * 8);
        prim::dev_memset(sel, 0, nw * 8);
        prim::for_each(F.R, RepHeadFn{F.key.p, F.slf.p, n, hb}, "repeat.heads");
        prim::for_each(F.k, RepSepFn{L.frc.p, F.key.p, F.slf.p, n, hb}, "repeat.separators");
        (void)prim::exclusive_scan<idx_t>(nw, PopcIn{hb}, hrank.p, true, "repeat.head_ranks");
        const RepRowFn row{n, levels, ri.min_len, ri.max_len ? ri.max_len : ~0ull, RepHeads{hb, hrank.p}, flt};
#ifdef GRLBWT_PRIM_HIP
        if (tiles) {
            u64 st[5];
            prim::repeat_search<VT, RepRowFn>(n, tree.p, row, sel, st);
            ri.n_repeats = st[0]; ri.n_maximal = st[1]; ri.far_searches = st[2]; ri.longest = st[3]; ri.largest_count = st[4];
        } else
#endif
        {
            ri.n_repeats = prim::reduce_sum<u64>(n, RepStatIn<VT>{tree.p, row, 0}, "repeat.count");
            ri.n_maximal = prim::reduce_sum<u64>(n, RepStatIn<VT>{tree.p, row, 1}, "repeat.maximal");
            ri.longest = prim::reduce_max<u64>(n, RepStatIn<VT>{tree.p, row, 2}, "repeat.longest");
            ri.largest_count = prim::reduce_max<u64>(n, RepStatIn<VT>{tree.p, row, 3}, "repeat.largest");
            prim::bitvector_from_pred(n, RepSelPred<VT>{tree.p, row}, sel, "repeat.select");
        }
        ri.n_selected = (u64)prim::exclusive_scan<idx_t>(nw, PopcIn{sel}, L.brank.p, true, "repeat.select_ranks");
        prim::sync();
        F.rinfo = ri;
        n_repeats = ri.n_selected;
        if (table && ri.n_selected > capacity)
            throw prim::Error(-22, "fm repeats: " + std::to_string(ri.n_selected) + " repeats, more than the output arrays hold");
        if (!table || ri.n_selected == 0) return;
        prim::for_each_set_bit<idx_t>(n, sel, L.brank.p, RepEmitFn<VT>{tree.p, row, lo, count, len, split}, "repeat.emit");
        prim::sync();
    }
    static void fm_repeats(const FmIndex &F, u64 min_len, u64 max_len, u64 min_count, u64 max_count, u32 flags, u64 row_begin, u64 row_end, u64 *lo,
                           u64 *count, u64 *len, u64 *split, u64 capacity, u64 &n_repeats, bool want_n) {
        n_repeats = 0;
        if (flags & ~kRepMaximal) throw prim::Error(-22, "fm repeats: unknown flag bits " + std::to_string(flags & ~kRepMaximal));
        if (min_len == 0) min_len = 1;
        if (max_len && max_len < min_len)
            throw prim::Error(-22, "fm repeats: max_len " + std::to_string(max_len) + " is below min_len " + std::to_string(min_len));
        const u64 n = F.n;
        if (row_end > n) row_end = n;                            // (UINT64_MAX: n_rows)
        if (row_begin > row_end)
            throw prim::Error(-22, "fm repeats: rows [" + std::to_string(row_begin) + ", " + std::to_string(row_end) + ") are no window of " + std::to_string(n) + " rows");
        const bool table = lo || count || len || split;
        if (!table && !want_n) throw prim::Error(-22, "fm repeats: no output");
        if (((uintptr_t)lo | (uintptr_t)count | (uintptr_t)len | (uintptr_t)split) & 7) throw prim::Error(-22, "fm repeats: an output is not aligned to 8 bytes");
        RepeatInfo ri;
        ri.n = n; ri.n_strings = F.k; ri.min_len = min_len; ri.max_len = max_len;
        if (n == 0) { F.rinfo = ri; return; }
        // the values: min(LCP, cap) with cap = max_len + 1, in the narrowest width that holds cap; without max_len whole, in 4 or 8 bytes
        const u64 lim = n >> 32 ? ~0ull : 0xFFFFFFFFull;
        const u64 cap = max_len && max_len < lim ? max_len + 1 : lim;
        const int vb = cap <= 0xFFull ? 1 : cap <= 0xFFFFull ? 2 : cap <= 0xFFFFFFFFull ? 4 : 8;
        ri.value_bytes = (u64)vb; ri.tree_levels = rep_levels(n);
        const u64 nw = FmLcp::words_of(n);
        ri.scratch_bytes = FmLcp::scratch_bytes(n) + rep_entries(n) * (u64)vb + (nw + 1) * sizeof(idx_t) + (n / kRepTileRows + 1) * 4 * 5 * 8;
        if (n >= ((u64)1 << 62) || ri.scratch_bytes > prim::mem_available())
            throw prim::Error(-12, "fm repeats: the passes need " + std::to_string(ri.scratch_bytes) + " bytes of device memory, more than is free");
        const RepFilter flt{row_begin, row_end, min_count > 2 ? min_count : 2, max_count ? max_count : ~0ull, (flags & kRepMaximal) != 0};
        FmLcp L;
        L.alloc(F);
        switch (vb) {
            case 1: fm_repeats_t<u8>(F, L, ri, flt, cap, lo, count, len, split, capacity, table, n_repeats); break;
            case 2: fm_repeats_t<u16>(F, L, ri, flt, cap, lo, count, len, split, capacity, table, n_repeats); break;
            case 4: fm_repeats_t<u32>(F, L, ri, flt, cap, lo, count, len, split, capacity, table, n_repeats); break;
            default: fm_repeats_t<u64>(F, L, ri, flt, cap, lo, count, len, split, capacity, table, n_repeats); break;
        }
    }
    static void fm_locate(const FmIndex &F, const u64 *rows, u64 nr, u64 max_steps, u64 *str, u64 *ofs) {
        if (!F.locate) throw prim::Error(-22, "fm locate: the index was made without the structures for locating");
        if (nr == 0) return;
        if (prim::reduce_sum<u64>(nr, FmRowBadIn{rows, F.n}, "fm.rows")) throw prim::Error(-22, "fm locate: a row is not below the number of symbols");
        const u64 lim = max_steps < F.n ? max_steps : F.n;
        if (F.checkpoints) prim::for_each(nr, FmLocateCpFn{F.lf(), F.sid.p, F.smp.p, F.cp, F.sep, lim, rows, str, ofs}, "fm.locate_cp");
        else prim::for_each(nr, FmLocateFn{F.lf(), F.sid.p, F.sep, lim, rows, str, ofs}, "fm.locate");
        prim::sync();
    }
    // ---- the document array and the suffix array (functor block "the document array and the suffix array").
    // Everything that can refuse the call runs before the first store: the arguments, then the strings' lengths -- the head
    // samples (form 1), the start positions of an index that extracts, or a length pass (form 0, only where offsets are written)
    // -- whose maximum has to fit the offsets' width.  Then one storing walk.  Rows on no string's chain (an image that is not
    // the BWT of a collection, accepted where the strings' own walks end) have no position: where the lengths do not add up to
    // n the window is first filled with FmLocateFn's "none", all bits set.  Without offsets on an index without checkpoints the
    // lengths are known only after the walk: the fill and a second walk follow it then.
    //   Loops: every walk is bounded by n steps (and ends sooner: fm_create has walked every string); nothing waits for another
    //   thread, and the only atomics are the ticket word's.
    template <class G>
    static void sa_width(int w, G g) {
        switch (w) {
        case 0: g(std::integral_constant<int, 0>{}); break;
        case 1: g(std::integral_constant<int, 1>{}); break;
        case 2: g(std::integral_constant<int, 2>{}); break;
        case 4: g(std::integral_constant<int, 4>{}); break;
        default: g(std::integral_constant<int, 8>{}); break;
        }
    }
    static void fm_sa(const FmIndex &F, u64 row_begin, u64 row_end, int ws, void *str, int wo, void *ofs) {
        if (!str && !ofs) throw prim::Error(-22, "fm sa: no output");
        if (!str) ws = 0;
        if (!ofs) wo = 0;
        const auto width_ok = [](int w) { return w == 1 || w == 2 || w == 4 || w == 8; };
        if (str && !width_ok(ws)) throw prim::Error(-22, "fm sa: string_bytes is " + std::to_string(ws) + ", not 1, 2, 4 or 8");
        if (ofs && !width_ok(wo)) throw prim::Error(-22, "fm sa: offset_bytes is " + std::to_string(wo) + ", not 1, 2, 4 or 8");
        if (!F.locate) throw prim::Error(-22, "fm sa: the index was made without the structures for locating");
        const u64 n = F.n, k = F.k;
        if (row_end == ~0ull) row_end = n;
        if (row_begin > row_end || row_end > n)
            throw prim::Error(-22, "fm sa: rows [" + std::to_string(row_begin) + ", " + std::to_string(row_end) + ") are no window of " + std::to_string(n) + " rows");
        if ((str && ((uintptr_t)str & (uintptr_t)(ws - 1))) || (ofs && ((uintptr_t)ofs & (uintptr_t)(wo - 1))))
            throw prim::Error(-22, "fm sa: an output is not aligned to its width");
        const auto fits = [](u64 v, int w) { return w == 8 || !(v >> (8 * w)); };
        if (str && k && !fits(k - 1, ws))
            throw prim::Error(-22, "fm sa: string number " + std::to_string(k - 1) + " does not fit string_bytes = " + std::to_string(ws));
        SaInfo si;
        si.n = n; si.k = k; si.row_begin = row_begin; si.row_end = row_end; si.string_bytes = (u64)ws; si.offset_bytes = (u64)wo;
        si.written = row_end - row_begin; si.form = F.checkpoints ? 1 : 0;
        if (row_end == row_begin) { F.sinfo = si; return; }      // (nothing to store: no walk)
        const u64 tickets = F.checkpoints ? F.walk.m : k;
        const bool from_starts = !F.checkpoints && wo && F.extract, len_pass = !F.checkpoints && wo && !F.extract;
        si.scratch_bytes = (tickets + (from_starts || len_pass ? k : 0)) * sizeof(idx_t) + 16;
        if (si.scratch_bytes > prim::mem_available())
            throw prim::Error(-12, "fm sa: the walks need " + std::to_string(si.scratch_bytes) + " bytes of device memory, more than is free");
        DBuf<idx_t> wsteps(tickets), slen;
        WalkInfo wi;
        u64 covered = ~0ull, longest = 0;                        // (covered: the rows on the strings' chains, once known)
        if (F.checkpoints) {
            covered = prim::reduce_sum<u64>(k, SaHeadLenIn{F.smp.p}, "sa.lengths");
            longest = prim::reduce_max<u64>(k, SaHeadLenIn{F.smp.p}, "sa.longest");
        } else if (wo) {
            slen.alloc(k);
            if (from_starts) prim::for_each(k, SaStartLenFn{F.T.p, slen.p}, "sa.lengths");
            else walk(k, SaLenFn{F.lf(), F.sep, n, slen.p}, wi, "sa.length_pass");
            covered = prim::reduce_sum<u64>(k, IdxIn64{slen.p}, "sa.lengths");
            longest = prim::reduce_max<u64>(k, IdxIn64{slen.p}, "sa.longest");
            if (len_pass) si.steps = covered - k;
        }
        if (wo && longest && !fits(longest - 1, wo))
            throw prim::Error(-22, "fm sa: offset " + std::to_string(longest - 1) + " of the longest string does not fit offset_bytes = " + std::to_string(wo));
        const SaWindow win{row_begin, row_end - row_begin};
        const auto none = [&] {                                  // FmLocateFn's answer for a row without a position
            if (str) prim::dev_memset(str, 0xFF, win.len * (u64)ws);
            if (ofs) prim::dev_memset(ofs, 0xFF, win.len * (u64)wo);
        };
        const auto store = [&] {
            sa_width(ws, [&](auto a) {
                sa_width(wo, [&](auto b) {
                    constexpr int WS = decltype(a)::value, WO = decltype(b)::value;
                    if constexpr (WS != 0 || WO != 0) {
                        SaOut<WS> so; SaOut<WO> oo;
                        if constexpr (WS != 0) so.p = (typename SaCell<WS>::type *)str;
                        if constexpr (WO != 0) oo.p = (typename SaCell<WO>::type *)ofs;
                        if (F.checkpoints) walk(tickets, SaSegFn<WS, WO>{F.lf(), F.sep, F.cp, F.smp.p, win, so, oo, wsteps.p}, wi, "sa.segments");
                        else walk(tickets, SaStringFn<WS, WO>{F.lf(), F.sep, n, slen.p, win, so, oo, wsteps.p}, wi, "sa.strings");
                    }
                });
            });
        };
        if (covered != ~0ull && covered != n) none();
        store();
        const u64 steps = prim::reduce_sum<u64>(tickets, IdxIn64{wsteps.p}, "sa.steps");
        if (covered == ~0ull && steps + k != n) { none(); store(); si.steps += steps; }
        si.steps += steps;
        si.longest = prim::reduce_max<u64>(tickets, IdxIn64{wsteps.p}, "sa.longest_walk");
        si.lanes = wi.lanes; si.refills = wi.refills;
        prim::sync();
        F.sinfo = si;
    }
    // ---- the compacted de Bruijn graph (functor block "the compacted de Bruijn graph").  debruijn_create does all
    // the work and keeps no pointer into the index; the three writers copy, and the cells of the unitigs are decoded from the
    // index again.  Everything that can refuse the create runs before anything is handed out: the arguments, the memory, the
    // passes (an image that is not the BWT of a collection).
    //   Device form: both passes of the edge search through prim::top_search (kDbTileNodes lanes of a workgroup on consecutive
    //   nodes under the LDS top level, every lane storing its node's entries: with about one in-edge per node they are consecutive
    //   entries; the staged tile kernel measured slower and is not kept, prim_hip.hpp) and prim::db_first_cells (a tile of
    //   kDbTileCells output cells per workgroup, one search per tile for its unitigs).  The stand-in runs the same functors
    //   through for_each; its form of the first cells, a for_each over the nodes, is the device's with GRLBWT_DEV_DEBRUIJN=f.
    //   Loops: the passes of fm_kmers; at most sigma symbols per node and pass; at most 2 (ceil(log2 n_nodes) + 1) jumping rounds,
    //   each one launch; k - 1 forward steps per unitig.  Nothing waits for another thread; the only atomics are the integer
    //   adds of out_degree and the flag of the second pass.
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kDbTileNodes = prim::kDbTileNodes, kDbTileCells = prim::kDbTileCells;
#else
    static constexpr u64 kDbTileNodes = 1024, kDbTileCells = 4096;      // (the serial form has no tiles: the figures the device library reports)
#endif
    struct DeBruijnInfo {
        u64 k = 0, n = 0, n_strings = 0, n_distinct = 0, n_nodes = 0, n_edges = 0, n_unitigs = 0, n_circular = 0, longest = 0, n_cells = 0;
        u64 max_in = 0, max_out = 0, passes = 0, length_passes = 0, backward_steps = 0, jump_rounds = 0, scratch_bytes = 0;
    };
    struct ImageDeBruijn {
        DeBruijnInfo i;
        u64 R = 0, sigma = 0, print = 0;          // of the index it was made from
        DBuf<idx_t> lo, count, unitig, rank, inoff, from, weight, row, uoff, uweight;
        DBuf<u32> indeg, outdeg;
        DBuf<u8> ucirc;
        u64 held_bytes() const {
            return (lo.n + count.n + unitig.n + rank.n + inoff.n + from.n + weight.n + row.n + uoff.n + uweight.n) * sizeof(idx_t) +
                   (indeg.n + outdeg.n) * 4 + ucirc.n;
        }
    };
    static u64 debruijn_print(const FmIndex &F) { return F.R ? prim::reduce_sum<u64>(F.R, DbPrintIn{F.key.p, F.slf.p}, "debruijn.fingerprint") : 0; }
    static void debruijn_create(const FmIndex &F, u64 k, u64 min_count, u64 max_count, u32 flags, ImageDeBruijn &D) {
        if (k == 0) throw prim::Error(-22, "de bruijn: k is 0");
        if (flags) throw prim::Error(-22, "de bruijn: unknown flag bits " + std::to_string(flags));
        if (max_count && min_count > max_count)
            throw prim::Error(-22, "de bruijn: min_count " + std::to_string(min_count) + " is above max_count " + std::to_string(max_count));
        const u64 n = F.n;
        DeBruijnInfo &di = D.i;
        di = DeBruijnInfo();
        di.k = k; di.n = n; di.n_strings = F.k;
        D.R = F.R; D.sigma = F.sigma;
        if (n == 0) return;
        di.scratch_bytes = KmerSel::scratch_bytes(n);
        if (n >= ((u64)1 << 62) || di.scratch_bytes > prim::mem_available())
            throw prim::Error(-12, "de bruijn: the passes need " + std::to_string(di.scratch_bytes) + " bytes of device memory, more than is free");
        D.print = debruijn_print(F);
        u64 nn = 0, ne = 0;
        {
            KmerSel K;
            KmerInfo ki;
            K.heads(F, k, ki);
            di.passes = ki.passes; di.length_passes = ki.length_passes;
            di.n_distinct = prim::reduce_sum<u64>((n + 63) / 64, PopcIn{K.H}, "debruijn.heads_sum");
            K.select(KmerFilter{0, n, min_count ? min_count : 1, max_count ? max_count : ~0ull}, ki);
            di.n_nodes = nn = ki.n_selected;
            if (nn == 0) { prim::sync(); return; }
            // per node: the handle's seven arrays and the steps of the first pass; then the jumping's eight arrays and two bytes
            const u64 node_bytes = nn * (6 * sizeof(idx_t) + 8) + nn * (sizeof(idx_t) + 4);
            const u64 jump_bytes = nn * (10 * sizeof(idx_t) + 2 + 8);
            di.scratch_bytes += jump_bytes > nn * (sizeof(idx_t) + 4) ? jump_bytes : nn * (sizeof(idx_t) + 4);
            if (node_bytes + jump_bytes > prim::mem_available())
                throw prim::Error(-12, "de bruijn: the graph needs " + std::to_string(node_bytes + jump_bytes) + " bytes of device memory, more than is free");
            D.lo.alloc(nn); D.count.alloc(nn);
            prim::for_each_set_bit<idx_t>(n, K.sel, K.L.brank.p, DbNodeFn{K.cnt(), D.lo.p, D.count.p}, "debruijn.nodes");
            D.indeg.alloc(nn); D.outdeg.alloc(nn);
            D.outdeg.zero();
            DBuf<idx_t> nsteps(nn);
            DBuf<u32> bad(1);
            bad.zero();
            DbEdgeFn f{F.key.p, F.slf.p, F.R, F.sep, DbPrevBit{K.B, K.NZ.p, K.nzbase.p, K.nzlist.p}, K.sel, K.L.brank.p, D.lo.p, D.count.p,
                       D.indeg.p, D.outdeg.p, nsteps.p, nullptr, bad.p};
#ifdef GRLBWT_PRIM_HIP
            prim::top_search(nn, f, F.top_entries, "debruijn.count");
#else
            prim::for_each(nn, DbEdgeLaneFn{f, DbGlobalSink{nullptr, nullptr, nullptr}}, "debruijn.count");
#endif
            ne = prim::reduce_sum<u64>(nn, DbDegIn{D.indeg.p}, "debruijn.edges_sum");
            if (ne > n) throw prim::Error(-22, "de bruijn: more windows of k + 1 cells than rows: not the BWT of a collection");
            di.n_edges = ne;
            if (ne * 3 * sizeof(idx_t) > prim::mem_available())
                throw prim::Error(-12, "de bruijn: the edges need " + std::to_string(ne * 3 * sizeof(idx_t)) + " bytes of device memory, more than is free");
            D.inoff.alloc(nn + 1);
            (void)prim::exclusive_scan<idx_t>(nn, DbDegIn{D.indeg.p}, D.inoff.p, true, "debruijn.in_offsets");
            D.from.alloc(ne); D.weight.alloc(ne); D.row.alloc(ne);
            f.inoff = D.inoff.p;
            const DbGlobalSink sink{D.from.p, D.weight.p, D.row.p};
#ifdef GRLBWT_PRIM_HIP
            prim::top_search(nn, DbEdgeLaneFn{f, sink}, F.top_entries, "debruijn.edges");
#else
            prim::for_each(nn, DbEdgeLaneFn{f, sink}, "debruijn.edges");
#endif
            if (bad.get(0)) throw prim::Error(-71, "de bruijn: a node's second pass found another number of edges than its first");
            di.backward_steps = 2 * prim::reduce_sum<u64>(nn, IdxIn64{nsteps.p}, "debruijn.steps");
            di.max_in = prim::reduce_max<u64>(nn, DbDegIn{D.indeg.p}, "debruijn.max_in");
            di.max_out = prim::reduce_max<u64>(nn, DbDegIn{D.outdeg.p}, "debruijn.max_out");
        }
        // the unitigs
        DBuf<idx_t> link(nn), succ(nn), p0(nn), d0(nn), m0(nn), p1(nn), d1(nn), m1(nn);
        DBuf<u8> mark(nn), open(nn);
        succ.fill_ff();
        prim::for_each(nn, DbLinkFn{D.indeg.p, D.outdeg.p, D.inoff.p, D.from.p, link.p, succ.p}, "debruijn.links");
        prim::for_each(nn, DbMarkFn{link.p, mark.p}, "debruijn.heads");
        prim::for_each(nn, DbJumpInitFn{link.p, mark.p, nullptr, p0.p, d0.p, m0.p}, "debruijn.jump_init");
        const u64 max_rounds = (u64)bitlen64(nn - 1) + 1;       // ceil(log2 n_nodes) + 1
        idx_t *P = p0.p, *Dd = d0.p, *M = m0.p, *Pn = p1.p, *Dn = d1.p, *Mn = m1.p;
        const auto rounds = [&]() {                              // returns the nodes that have found no head
            u64 left = prim::reduce_sum<u64>(nn, DbOpenIn{mark.p, P}, "debruijn.open");
            for (u64 r = 0; r < max_rounds && left; r++) {
                prim::for_each(nn, DbJumpFn{mark.p, P, Dd, M, Pn, Dn, Mn}, "debruijn.jump");
                std::swap(P, Pn); std::swap(Dd, Dn); std::swap(M, Mn);
                di.jump_rounds++;
                left = prim::reduce_sum<u64>(nn, DbOpenIn{mark.p, P}, "debruijn.open");
            }
            return left;
        };
        if (rounds()) {                                          // what is left lies on cycles: their smallest nodes become heads
            prim::for_each(nn, DbOpenFn{mark.p, P, open.p}, "debruijn.cycle_nodes");
            prim::for_each(nn, DbCycleHeadFn{open.p, M, mark.p}, "debruijn.cycle_heads");
            prim::for_each(nn, DbJumpInitFn{link.p, mark.p, open.p, P, Dd, M}, "debruijn.cycle_init");
            if (rounds()) throw prim::Error(-71, "de bruijn: nodes without a unitig after the cycle rounds");
        }
        DBuf<idx_t> hrank(nn + 1);
        const u64 nu = (u64)prim::exclusive_scan<idx_t>(nn, DbMarkIn{mark.p, 0}, hrank.p, true, "debruijn.unitig_ids");
        di.n_unitigs = nu;
        di.n_circular = prim::reduce_sum<u64>(nn, DbMarkIn{mark.p, 2}, "debruijn.circular");
        D.unitig.alloc(nn); D.rank.alloc(nn); D.ucirc.alloc(nu);
        DBuf<idx_t> ulen(nu);
        prim::for_each(nn, DbPlaceFn{mark.p, P, Dd, hrank.p, succ.p, D.unitig.p, D.rank.p, ulen.p, D.ucirc.p}, "debruijn.place");
        D.uoff.alloc(nu + 1);
        (void)prim::exclusive_scan<idx_t>(nu, IdxIn<idx_t>{ulen.p}, D.uoff.p, true, "debruijn.node_offsets");
        di.longest = prim::reduce_max<u64>(nu, IdxIn64{ulen.p}, "debruijn.longest");
        {
            idx_t *nodes = Pn;                                   // (a spare generation of the rounds)
            DBuf<u64> wsum(nn + 1);
            prim::for_each(nn, DbOrderFn{D.unitig.p, D.rank.p, D.uoff.p, nodes}, "debruijn.order");
            (void)prim::exclusive_scan<u64>(nn, DbCountOfIn{nodes, D.count.p}, wsum.p, true, "debruijn.weights_scan");
            D.uweight.alloc(nu);
            prim::for_each(nu, DbWeightFn{D.uoff.p, wsum.p, D.uweight.p}, "debruijn.weights");
        }
        di.n_cells = nn + nu * (k - 1);
        prim::sync();
    }
    template <class S>
    static void debruijn_copy(const S *src, u64 *dst, u64 m, const char *name) { if (dst && m) prim::for_each(m, DbCopyFn<S, u64>{src, dst}, name); }
    static void debruijn_nodes(const ImageDeBruijn &D, u64 *lo, u64 *count, u32 *indeg, u32 *outdeg, u64 *unitig, u64 *rank, u64 capacity) {
        if (!lo && !count && !indeg && !outdeg && !unitig && !rank) throw prim::Error(-22, "de bruijn nodes: no output");
        const u64 nn = D.i.n_nodes;
        if (capacity < nn) throw prim::Error(-22, "de bruijn nodes: " + std::to_string(nn) + " nodes, more than the output arrays hold");
        if ((((uintptr_t)lo | (uintptr_t)count | (uintptr_t)unitig | (uintptr_t)rank) & 7) || (((uintptr_t)indeg | (uintptr_t)outdeg) & 3))
            throw prim::Error(-22, "de bruijn nodes: an output is not aligned to its width");
        debruijn_copy(D.lo.p, lo, nn, "debruijn.copy_lo");
        debruijn_copy(D.count.p, count, nn, "debruijn.copy_count");
        debruijn_copy(D.unitig.p, unitig, nn, "debruijn.copy_unitig");
        debruijn_copy(D.rank.p, rank, nn, "debruijn.copy_rank");
        if (indeg && nn) prim::d2d(indeg, D.indeg.p, nn * 4);
        if (outdeg && nn) prim::d2d(outdeg, D.outdeg.p, nn * 4);
        prim::sync();
    }
    static void debruijn_edges(const ImageDeBruijn &D, u64 *inoff, u64 *from, u64 *weight, u64 *row, u64 capacity) {
        if (!inoff && !from && !weight && !row) throw prim::Error(-22, "de bruijn edges: no output");
        const u64 nn = D.i.n_nodes, ne = D.i.n_edges;
        if (capacity < ne)
            throw prim::Error(-22, "de bruijn edges: " + std::to_string(ne) + " edges, more than the output arrays hold");
        if (((uintptr_t)inoff | (uintptr_t)from | (uintptr_t)weight | (uintptr_t)row) & 7) throw prim::Error(-22, "de bruijn edges: an output is not aligned to 8 bytes");
        if (inoff) { if (nn) debruijn_copy(D.inoff.p, inoff, nn + 1, "debruijn.copy_in_offsets"); else prim::dev_memset(inoff, 0, 8); }
        debruijn_copy(D.from.p, from, ne, "debruijn.copy_from");
        debruijn_copy(D.weight.p, weight, ne, "debruijn.copy_weight");
        debruijn_copy(D.row.p, row, ne, "debruijn.copy_row");
        prim::sync();
    }
    static void debruijn_unitigs(const ImageDeBruijn &D, const FmIndex *F, int w, u64 *uoff, u64 *nodes, void *cells, u64 *weight, u8 *circ, u64 cap_u,
                                 u64 cap_n, u64 cap_c) {
        if (!uoff && !nodes && !cells && !weight && !circ) throw prim::Error(-22, "de bruijn unitigs: no output");
        const u64 nn = D.i.n_nodes, nu = D.i.n_unitigs, nc = D.i.n_cells, k = D.i.k;
        if ((uoff || weight || circ) && cap_u < nu)
            throw prim::Error(-22, "de bruijn unitigs: " + std::to_string(nu) + " unitigs, more than the output arrays hold");
        if (nodes && cap_n < nn) throw prim::Error(-22, "de bruijn unitigs: " + std::to_string(nn) + " nodes, more than the output array holds");
        if (cells && cap_c < nc) throw prim::Error(-22, "de bruijn unitigs: " + std::to_string(nc) + " cells, more than the output array holds");
        if (((uintptr_t)uoff | (uintptr_t)nodes | (uintptr_t)weight) & 7) throw prim::Error(-22, "de bruijn unitigs: an output is not aligned to 8 bytes");
        if (cells) {
            if (!(w == 1 || w == 2 || w == 4 || w == 8)) throw prim::Error(-22, "de bruijn unitigs: cell_bytes is " + std::to_string(w) + ", not 1, 2, 4 or 8");
            if ((uintptr_t)cells & (uintptr_t)(w - 1)) throw prim::Error(-22, "de bruijn unitigs: an output is not aligned to its width");
            if (!F) throw prim::Error(-22, "de bruijn unitigs: the cells need the index the graph was made from");
            if (F->n != D.i.n || F->R != D.R || F->k != D.i.n_strings || F->sigma != D.sigma || (F->n && debruijn_print(*F) != D.print))
                throw prim::Error(-22, "de bruijn unitigs: not the index the graph was made from");
            if (w < 8 && F->R) {
                const u64 top = F->alpha.p ? F->alpha.get(F->alpha.n - 1) : (u64)F->key.get(F->R - 1).host_sym();
                if (top >> (8 * w))
                    throw prim::Error(-22, "de bruijn unitigs: the image's largest symbol " + std::to_string(top) + " does not fit cell_bytes = " + std::to_string(w));
            }
        }
        if (uoff) { if (nu) debruijn_copy(D.uoff.p, uoff, nu + 1, "debruijn.copy_node_offsets"); else prim::dev_memset(uoff, 0, 8); }
        debruijn_copy(D.uweight.p, weight, nu, "debruijn.copy_unitig_weight");
        if (circ && nu) prim::d2d(circ, D.ucirc.p, nu);
        if ((nodes || cells) && nn) {
            DBuf<idx_t> order(nn);
            prim::for_each(nn, DbOrderFn{D.unitig.p, D.rank.p, D.uoff.p, order.p}, "debruijn.order");
            debruijn_copy(order.p, nodes, nn, "debruijn.copy_nodes");
            if (cells) {
                DBuf<RankCell> frc;
                fm_run_cells(*F, frc);
                const KmerStepFn step{frc.p, F->key.p, F->slf.p, F->alpha.p};
                with_cell(w, [&](auto c) {
                    typedef decltype(c) cell_t;
#ifdef GRLBWT_PRIM_HIP
                    if (prim::sw().dev_debruijn != 'f') prim::db_first_cells<cell_t, idx_t>(nc, nu, k, D.uoff.p, order.p, D.lo.p, step, (cell_t *)cells);
                    else
#endif
                        prim::for_each(nn, DbFirstCellFn<cell_t>{step, order.p, D.unitig.p, D.lo.p, k, (cell_t *)cells}, "debruijn.first_cells_plain");
                    if (k > 1) prim::for_each(nu, DbTailCellsFn<cell_t>{step, order.p, D.uoff.p, D.lo.p, k, (cell_t *)cells}, "debruijn.tail_cells");
                });
            }
        }
        prim::sync();
    }
    // ---- the strand-merged compacted de Bruijn graph (functor block of that name).  cdebruijn_create does all the
    // work and keeps no pointer into the index; the three writers copy, and the cells are decoded from the index again behind
    // the fingerprint check.  Order of events: the arguments and the complement map; the memory of the passes; the passes and the
    // mate pass (CkSel, shared with fm_ckmers, whose info record this call leaves alone); the selection by total; the memory of
    // the nodes and heads; the edge search from every selected head, count then emit; the memory of the sort; the two sorts and
    // the merge; the memory of the rounds; the unitigs on the doubled graph.
    //   Device form: the mate pass and the edge search as in 4o and 4n; prim::cdb_merge (a tile of sorted records per workgroup:
    //   group heads as ballot words, the tile's entries stored behind one scan) and prim::cdb_first_cells (a tile of consecutive
    //   cells per workgroup, one search per tile for its unitigs) with the walks of the - nodes without a mate as tickets
    //   (prim::walk_tickets).  Generic forms, the stand-in's and with GRLBWT_DEV_CDEBRUIJN=f the device's: for_each over the
    //   sorted records behind a scan of the flags; for_each over the nodes with the walks inline.
    //   Loops: those of fm_ckmers and debruijn_create; the jumping runs on 2 n_nodes oriented nodes, at most
    //   2 (ceil(log2(2 n_nodes)) + 1) rounds.  Nothing waits for another thread; the only atomics are the flags' and the tickets'.
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kCdbTileNodes = prim::kDbTileNodes, kCdbTileCells = prim::kCdbTileCells;
#else
    static constexpr u64 kCdbTileNodes = 1024, kCdbTileCells = 4096;    // (the serial form has no tiles: the figures the device library reports)
#endif
    struct CDeBruijnInfo {
        u64 k = 0, n = 0, n_strings = 0, n_distinct = 0, n_nodes = 0, n_rigid = 0, n_palindromes = 0, n_edges = 0, n_half_edges = 0, n_hairpins = 0;
        u64 n_unitigs = 0, n_circular = 0, longest = 0, n_cells = 0, max_end_degree = 0, passes = 0, length_passes = 0;
        u64 mate_backward_steps = 0, edge_backward_steps = 0, forward_steps = 0, jump_rounds = 0, scratch_bytes = 0;
    };
    struct ImageCDeBruijn {
        CDeBruijnInfo i;
        mutable u64 cells_forward_steps = 0;      // of the last unitigs call that wrote cells
        u64 R = 0, sigma = 0, print = 0;          // of the index it was made from
        u64 n_walk = 0, comp_top = 0;             // - nodes without a mate; the largest complement value of the table
        u32 nt = 0;
        DBuf<idx_t> lo, count, mate, total, unitig, rank, endoff, eoth, ew, erow, ecnt, uoff, uweight;
        DBuf<u8> orient, ucirc;
        DBuf<u32> ccode;
        DBuf<u64> cval;
        u64 held_bytes() const {
            return (lo.n + count.n + mate.n + total.n + unitig.n + rank.n + endoff.n + eoth.n + ew.n + erow.n + ecnt.n + uoff.n + uweight.n) * sizeof(idx_t) +
                   orient.n + ucirc.n + ccode.n * 4 + cval.n * 8;
        }
    };
    static void cdb_need(u64 bytes, const char *what) {
        if (bytes > prim::mem_available())
            throw prim::Error(-12, std::string("canonical de bruijn: ") + what + " need " + std::to_string(bytes) + " bytes of device memory, more than is free");
    }
    static void cdebruijn_create(const FmIndex &F, u64 k, u64 min_count, u64 max_count, const u64 *host_pairs, u64 n_pairs, u32 flags, ImageCDeBruijn &D) {
        static const char *const kWho = "canonical de bruijn: ";
        if (k == 0) throw prim::Error(-22, std::string(kWho) + "k is 0");
        if (flags) throw prim::Error(-22, std::string(kWho) + "unknown flag bits " + std::to_string(flags));
        if (max_count && min_count > max_count)
            throw prim::Error(-22, std::string(kWho) + "min_count " + std::to_string(min_count) + " is above max_count " + std::to_string(max_count));
        CkSel S;
        S.pairs(kWho, F, host_pairs, n_pairs);
        const u64 n = F.n;
        CDeBruijnInfo &di = D.i;
        di = CDeBruijnInfo();
        di.k = k; di.n = n; di.n_strings = F.k;
        D.R = F.R; D.sigma = F.sigma;
        if (n == 0) return;
        const u64 nw = FmLcp::words_of(n);
        di.scratch_bytes = KmerSel::scratch_bytes(n) + (nw + 1) * sizeof(idx_t) + S.fixed_bytes();
        if (n >= ((u64)1 << 62) || di.scratch_bytes > prim::mem_available())
            throw prim::Error(-12, std::string(kWho) + "the passes need " + std::to_string(di.scratch_bytes) + " bytes of device memory, more than is free");
        D.print = debruijn_print(F);
        S.table(F);
        {   // the handle's own complement table: code -> the complement's value
            std::vector<std::pair<u32, u64>> t;
            for (u64 i = 0; i < S.n_pairs; i++) {
                const u32 a = S.codes[2 * i], b = S.codes[2 * i + 1];
                if (a != kCkAbsent) t.push_back({a, S.vals[2 * i + 1]});
                if (b != kCkAbsent && S.vals[2 * i] != S.vals[2 * i + 1]) t.push_back({b, S.vals[2 * i]});
            }
            std::sort(t.begin(), t.end());
            D.nt = (u32)t.size();
            std::vector<u32> cc(D.nt);
            std::vector<u64> cv(D.nt);
            for (u32 i = 0; i < D.nt; i++) { cc[i] = t[i].first; cv[i] = t[i].second; if (cv[i] > D.comp_top) D.comp_top = cv[i]; }
            D.ccode.alloc(D.nt); D.cval.alloc(D.nt);
            if (D.nt) { prim::h2d(D.ccode.p, cc.data(), D.nt * 4); prim::h2d(D.cval.p, cv.data(), D.nt * 8); }
        }
        KmerSel &K = S.K;
        KmerInfo ki;
        S.heads(F, k, ki);
        di.passes = ki.passes; di.length_passes = ki.length_passes;
        di.n_distinct = S.n_distinct;
        di.scratch_bytes += di.n_distinct * sizeof(idx_t);
        S.mates(kWho, F, k);
        di.mate_backward_steps = S.backward_steps; di.forward_steps = S.forward_steps;
        const CkRank rk{K.H, S.hrank.p};
        const CkTotalFn tot{K.cnt(), rk, S.mate.p};
        const u64 *rep = S.representatives();
        const u64 nn = K.select_classes(rep, tot, KmerFilter{0, n, min_count ? min_count : 1, max_count ? max_count : ~0ull});
        di.n_nodes = nn;
        if (nn == 0) { prim::sync(); return; }
        const u64 N2 = 2 * nn;
        if (N2 + 1 >= (u64)kCkNoComp) throw prim::Error(-75, std::string(kWho) + "more ends than positions of this width can number");
        // ---- the nodes and the selected heads
        cdb_need(nn * 4 * sizeof(idx_t) + (nw + nw + 1) * 8, "the nodes");
        D.lo.alloc(nn); D.count.alloc(nn); D.mate.alloc(nn); D.total.alloc(nn);
        prim::for_each_set_bit<idx_t>(n, K.sel, K.L.brank.p, CdbNodeFn{tot, D.lo.p, D.count.p, D.mate.p, D.total.p}, "cdebruijn.nodes");
        di.n_rigid = prim::reduce_sum<u64>(nn, CdbNodeKindIn{D.lo.p, D.mate.p, 0}, "cdebruijn.rigid");
        di.n_palindromes = prim::reduce_sum<u64>(nn, CdbNodeKindIn{D.lo.p, D.mate.p, 1}, "cdebruijn.palindromes");
        u64 nf = 0, nhe = 0;
        DBuf<idx_t> rsrc, roth, rlo, rocc;
        {
            const CdbHeadOf head{K.H, rk, S.mate.p, K.sel, K.L.brank.p};
            DBuf<u64> hsel(nw);
            DBuf<idx_t> hselrank(nw + 1);
            hsel.zero();
            prim::bitvector_from_pred(n, CdbHeadPred{head}, hsel.p, "cdebruijn.heads");
            const u64 nh = (u64)prim::exclusive_scan<idx_t>(nw, PopcIn{hsel.p}, hselrank.p, true, "cdebruijn.head_ranks");
            di.scratch_bytes += nw * 8 + (nw + 1) * sizeof(idx_t) + nh * 6 * sizeof(idx_t);
            cdb_need(nh * 6 * sizeof(idx_t), "the heads");
            DBuf<idx_t> hlo(nh), hcount(nh), hend(nh), found(nh), nsteps(nh), roff(nh + 1);
            prim::for_each_set_bit<idx_t>(n, hsel.p, hselrank.p, CdbHeadListFn{head, K.cnt(), hlo.p, hcount.p, hend.p}, "cdebruijn.head_list");
            DBuf<u32> bad(1);
            bad.zero();
            DbEdgeFn e{F.key.p, F.slf.p, F.R, F.sep, DbPrevBit{K.B, K.NZ.p, K.nzbase.p, K.nzlist.p}, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr};
            CdbEdgeFn f{e, head, hlo.p, hcount.p, hend.p, found.p, nsteps.p, nullptr, nullptr, nullptr, nullptr, nullptr, bad.p};
#ifdef GRLBWT_PRIM_HIP
            prim::top_search(nh, f, F.top_entries, "cdebruijn.count");
#else
            prim::for_each(nh, f, "cdebruijn.count");
#endif
            nf = (u64)prim::exclusive_scan<idx_t>(nh, IdxIn<idx_t>{found.p}, roff.p, true, "cdebruijn.record_offsets");
            if (nf > n) throw prim::Error(-22, std::string(kWho) + "more windows of k + 1 cells than rows: not the BWT of a collection");
            di.scratch_bytes += nf * 4 * sizeof(idx_t);
            cdb_need(nf * 4 * sizeof(idx_t), "the records");
            rsrc.alloc(nf); roth.alloc(nf); rlo.alloc(nf); rocc.alloc(nf);
            f.roff = roff.p; f.rsrc = rsrc.p; f.roth = roth.p; f.rlo = rlo.p; f.rocc = rocc.p;
#ifdef GRLBWT_PRIM_HIP
            prim::top_search(nh, f, F.top_entries, "cdebruijn.records");
#else
            prim::for_each(nh, f, "cdebruijn.records");
#endif
            if (bad.get(0)) throw prim::Error(-71, std::string(kWho) + "a head's second pass found another number of windows than its first");
            di.edge_backward_steps = 2 * prim::reduce_sum<u64>(nh, IdxIn64{nsteps.p}, "cdebruijn.steps");
        }
        // ---- the merge: two stable sorts of the record numbers, group heads, one entry per group
        D.endoff.alloc(N2 + 1);
        if (nf) {
            const u64 nrec = 2 * nf;
            di.n_hairpins = prim::reduce_sum<u64>(nf, CdbHairpinIn{rsrc.p, roth.p}, "cdebruijn.hairpins");
            di.scratch_bytes += nrec * 5 * sizeof(idx_t);
            cdb_need(nrec * 5 * sizeof(idx_t), "the sorts");
            const CdbRec rec{rsrc.p, roth.p, nf, N2};
            DBuf<idx_t> ka(nrec), va(nrec), kb(nrec), vb(nrec);
            const int bits = std::max((int)bitlen64(N2), 1);
            prim::for_each(nrec, CdbKeyFn{rec, nullptr, ka.p, va.p}, "cdebruijn.keys_other");
            int res = prim::sort_pairs<idx_t, idx_t>(ka.p, va.p, kb.p, vb.p, nrec, 0, bits, "cdebruijn.sort_other");
            idx_t *perm = res ? vb.p : va.p, *key = res ? kb.p : ka.p, *key2 = res ? ka.p : kb.p, *perm2 = res ? va.p : vb.p;      // (in: the side the first sort ended on)
            prim::for_each(nrec, CdbKeyFn{rec, perm, key, nullptr}, "cdebruijn.keys_source");
            res = prim::sort_pairs<idx_t, idx_t>(key, perm, key2, perm2, nrec, 0, bits, "cdebruijn.sort_source");
            if (res) std::swap(perm, perm2);
            idx_t *eidx = perm2;                                 // (the spare value array)
            const CdbGroupHeadIn gh{rec, perm};
            DBuf<idx_t> esrc;
            DBuf<u32> bad(1);
            bad.zero();
            CdbMerge merge{rec, perm, rlo.p, rocc.p, nrec, nullptr, nullptr, nullptr, nullptr, nullptr, bad.p};
            const auto entries = [&]() {
                cdb_need(nhe * 5 * sizeof(idx_t), "the half-edges");
                esrc.alloc(nhe); D.eoth.alloc(nhe); D.ew.alloc(nhe); D.erow.alloc(nhe); D.ecnt.alloc(nhe);
                merge.esrc = esrc.p; merge.eoth = D.eoth.p; merge.ew = D.ew.p; merge.erow = D.erow.p; merge.ecnt = D.ecnt.p;
            };
#ifdef GRLBWT_PRIM_HIP
            if (prim::sw().dev_cdebruijn != 'f') {
                prim::CdbFlags fl;
                nhe = prim::cdb_flags(nrec, gh, fl);
                entries();
                prim::cdb_merge(nrec, fl, merge);
            } else
#endif
            {
                nhe = prim::reduce_sum<u64>(nrec, gh, "cdebruijn.groups");
                entries();
                (void)prim::exclusive_scan<idx_t>(nrec, gh, eidx, false, "cdebruijn.group_ranks");
                prim::for_each(nrec, CdbMergeEachFn{gh, eidx, merge}, "cdebruijn.merge_plain");
            }
            if (bad.get(0)) throw prim::Error(-22, std::string(kWho) + "more than a window and its reverse complement between two ends: not the BWT of a collection");
            prim::for_each(N2 + 1, CdbEndOffFn{esrc.p, nhe, D.endoff.p}, "cdebruijn.end_offsets");
            const u64 self = prim::reduce_sum<u64>(nhe, CdbSelfIn{esrc.p, D.eoth.p}, "cdebruijn.self");
            if (self != di.n_hairpins || ((nhe + self) & 1))
                throw prim::Error(-22, std::string(kWho) + "half-edges without their reverse: not the BWT of a collection");
            di.n_half_edges = nhe; di.n_edges = (nhe + self) / 2;
            di.max_end_degree = prim::reduce_max<u64>(N2, CdbEndDegIn{D.endoff.p}, "cdebruijn.max_degree");
        } else {
            D.endoff.zero();
        }
        rsrc.release(); roth.release(); rlo.release(); rocc.release();
        // ---- the unitigs on the doubled graph: 4n's rounds over the 2 n_nodes oriented nodes
        di.scratch_bytes += N2 * (10 * sizeof(idx_t) + 3 + 8);
        cdb_need(N2 * (10 * sizeof(idx_t) + 3 + 8) + nn * (2 * sizeof(idx_t) + 1), "the rounds");
        DBuf<idx_t> link(N2), succ(N2), p0(N2), d0(N2), m0(N2), p1(N2), d1(N2), m1(N2);
        DBuf<u8> mark(N2), open(N2), keep(N2);
        keep.zero();
        const CdbEnds ends{D.endoff.p, D.eoth.p, D.lo.p, D.mate.p};
        prim::for_each(N2, CdbLinkFn{ends, link.p, succ.p}, "cdebruijn.links");
        prim::for_each(N2, DbMarkFn{link.p, mark.p}, "cdebruijn.heads_mark");
        prim::for_each(N2, DbJumpInitFn{link.p, mark.p, nullptr, p0.p, d0.p, m0.p}, "cdebruijn.jump_init");
        const u64 max_rounds = (u64)bitlen64(N2 - 1) + 1;
        idx_t *P = p0.p, *Dd = d0.p, *M = m0.p, *Pn = p1.p, *Dn = d1.p, *Mn = m1.p;
        const auto rounds = [&]() {
            u64 left = prim::reduce_sum<u64>(N2, DbOpenIn{mark.p, P}, "cdebruijn.open");
            for (u64 r = 0; r < max_rounds && left; r++) {
                prim::for_each(N2, DbJumpFn{mark.p, P, Dd, M, Pn, Dn, Mn}, "cdebruijn.jump");
                std::swap(P, Pn); std::swap(Dd, Dn); std::swap(M, Mn);
                di.jump_rounds++;
                left = prim::reduce_sum<u64>(N2, DbOpenIn{mark.p, P}, "cdebruijn.open");
            }
            return left;
        };
        if (rounds()) {
            prim::for_each(N2, DbOpenFn{mark.p, P, open.p}, "cdebruijn.cycle_nodes");
            prim::for_each(N2, DbCycleHeadFn{open.p, M, mark.p}, "cdebruijn.cycle_heads");
            prim::for_each(N2, DbJumpInitFn{link.p, mark.p, open.p, P, Dd, M}, "cdebruijn.cycle_init");
            if (rounds()) throw prim::Error(-71, std::string(kWho) + "nodes without a unitig after the cycle rounds");
        }
        prim::for_each(N2, CdbKeepFn{mark.p, P, succ.p, keep.p}, "cdebruijn.keep");
        DBuf<idx_t> hrank(N2 + 1);
        const u64 nu = (u64)prim::exclusive_scan<idx_t>(N2, CdbKeptIn{mark.p, keep.p, 0}, hrank.p, true, "cdebruijn.unitig_ids");
        di.n_unitigs = nu;
        di.n_circular = prim::reduce_sum<u64>(N2, CdbKeptIn{mark.p, keep.p, 2}, "cdebruijn.circular");
        D.unitig.alloc(nn); D.rank.alloc(nn); D.orient.alloc(nn); D.ucirc.alloc(nu);
        DBuf<idx_t> ulen(nu);
        prim::for_each(N2, CdbPlaceFn{mark.p, keep.p, P, Dd, hrank.p, succ.p, D.unitig.p, D.rank.p, ulen.p, D.orient.p, D.ucirc.p}, "cdebruijn.place");
        D.uoff.alloc(nu + 1);
        const u64 placed = (u64)prim::exclusive_scan<idx_t>(nu, IdxIn<idx_t>{ulen.p}, D.uoff.p, true, "cdebruijn.node_offsets");
        if (placed != nn) throw prim::Error(-71, std::string(kWho) + "the unitigs hold " + std::to_string(placed) + " nodes, not " + std::to_string(nn));
        di.longest = prim::reduce_max<u64>(nu, IdxIn64{ulen.p}, "cdebruijn.longest");
        {
            idx_t *nodes = Pn;                                   // (a spare generation of the rounds)
            DBuf<u64> wsum(nn + 1);
            prim::for_each(nn, CdbOrderFn{D.unitig.p, D.rank.p, D.uoff.p, D.orient.p, nodes}, "cdebruijn.order");
            (void)prim::exclusive_scan<u64>(nn, CdbTotalOfIn{nodes, D.total.p}, wsum.p, true, "cdebruijn.weights_scan");
            D.uweight.alloc(nu);
            prim::for_each(nu, DbWeightFn{D.uoff.p, wsum.p, D.uweight.p}, "cdebruijn.weights");
            D.n_walk = prim::reduce_sum<u64>(nn, CdbWalkIn{CdbWalkPred{CdbCellSrc{D.lo.p, D.mate.p}, nodes}}, "cdebruijn.walk_nodes");
        }
        di.n_cells = nn + nu * (k - 1);
        prim::sync();
    }
    static void cdebruijn_nodes(const ImageCDeBruijn &D, u64 *lo, u64 *count, u64 *mate_lo, u64 *total, u32 *deg0, u32 *deg1, u64 *unitig, u64 *rank, u8 *orient,
                                u64 capacity) {
        if (!lo && !count && !mate_lo && !total && !deg0 && !deg1 && !unitig && !rank && !orient) throw prim::Error(-22, "canonical de bruijn nodes: no output");
        const u64 nn = D.i.n_nodes;
        if (capacity < nn) throw prim::Error(-22, "canonical de bruijn nodes: " + std::to_string(nn) + " nodes, more than the output arrays hold");
        if ((((uintptr_t)lo | (uintptr_t)count | (uintptr_t)mate_lo | (uintptr_t)total | (uintptr_t)unitig | (uintptr_t)rank) & 7) || (((uintptr_t)deg0 | (uintptr_t)deg1) & 3))
            throw prim::Error(-22, "canonical de bruijn nodes: an output is not aligned to its width");
        debruijn_copy(D.lo.p, lo, nn, "cdebruijn.copy_lo");
        debruijn_copy(D.count.p, count, nn, "cdebruijn.copy_count");
        if (mate_lo && nn) prim::for_each(nn, CdbCopyMateFn{D.mate.p, mate_lo}, "cdebruijn.copy_mate_lo");
        debruijn_copy(D.total.p, total, nn, "cdebruijn.copy_total");
        debruijn_copy(D.unitig.p, unitig, nn, "cdebruijn.copy_unitig");
        debruijn_copy(D.rank.p, rank, nn, "cdebruijn.copy_rank");
        if ((deg0 || deg1) && nn) prim::for_each(nn, CdbDegreeFn{D.endoff.p, deg0, deg1}, "cdebruijn.copy_degrees");
        if (orient && nn) prim::d2d(orient, D.orient.p, nn);
        prim::sync();
    }
    static void cdebruijn_links(const ImageCDeBruijn &D, u64 *endoff, u64 *other, u64 *weight, u64 *row, u64 *cnt, u64 capacity) {
        if (!endoff && !other && !weight && !row && !cnt) throw prim::Error(-22, "canonical de bruijn links: no output");
        const u64 nn = D.i.n_nodes, nhe = D.i.n_half_edges;
        if (capacity < nhe) throw prim::Error(-22, "canonical de bruijn links: " + std::to_string(nhe) + " half-edges, more than the output arrays hold");
        if (((uintptr_t)endoff | (uintptr_t)other | (uintptr_t)weight | (uintptr_t)row | (uintptr_t)cnt) & 7)
            throw prim::Error(-22, "canonical de bruijn links: an output is not aligned to 8 bytes");
        if (endoff) { if (nn) debruijn_copy(D.endoff.p, endoff, 2 * nn + 1, "cdebruijn.copy_end_offsets"); else prim::dev_memset(endoff, 0, 8); }
        debruijn_copy(D.eoth.p, other, nhe, "cdebruijn.copy_other");
        debruijn_copy(D.ew.p, weight, nhe, "cdebruijn.copy_weight");
        if (row && nhe) prim::for_each(nhe, CdbCopyRowFn{D.erow.p, row}, "cdebruijn.copy_fwd_row");
        debruijn_copy(D.ecnt.p, cnt, nhe, "cdebruijn.copy_fwd_count");
        prim::sync();
    }
    static void cdebruijn_unitigs(const ImageCDeBruijn &D, const FmIndex *F, int w, u64 *uoff, u64 *nodes, void *cells, u64 *weight, u8 *circ, u64 cap_u,
                                  u64 cap_n, u64 cap_c) {
        static const char *const kWho = "canonical de bruijn unitigs: ";
        if (!uoff && !nodes && !cells && !weight && !circ) throw prim::Error(-22, std::string(kWho) + "no output");
        const u64 nn = D.i.n_nodes, nu = D.i.n_unitigs, nc = D.i.n_cells, k = D.i.k;
        if ((uoff || weight || circ) && cap_u < nu) throw prim::Error(-22, std::string(kWho) + std::to_string(nu) + " unitigs, more than the output arrays hold");
        if (nodes && cap_n < nn) throw prim::Error(-22, std::string(kWho) + std::to_string(nn) + " nodes, more than the output array holds");
        if (cells && cap_c < nc) throw prim::Error(-22, std::string(kWho) + std::to_string(nc) + " cells, more than the output array holds");
        if (((uintptr_t)uoff | (uintptr_t)nodes | (uintptr_t)weight) & 7) throw prim::Error(-22, std::string(kWho) + "an output is not aligned to 8 bytes");
        if (cells) {
            if (!(w == 1 || w == 2 || w == 4 || w == 8)) throw prim::Error(-22, std::string(kWho) + "cell_bytes is " + std::to_string(w) + ", not 1, 2, 4 or 8");
            if ((uintptr_t)cells & (uintptr_t)(w - 1)) throw prim::Error(-22, std::string(kWho) + "an output is not aligned to its width");
            if (!F) throw prim::Error(-22, std::string(kWho) + "the cells need the index the graph was made from");
            if (F->n != D.i.n || F->R != D.R || F->k != D.i.n_strings || F->sigma != D.sigma || (F->n && debruijn_print(*F) != D.print))
                throw prim::Error(-22, std::string(kWho) + "not the index the graph was made from");
            if (w < 8 && F->R) {
                u64 top = F->alpha.p ? F->alpha.get(F->alpha.n - 1) : (u64)F->key.get(F->R - 1).host_sym();
                if (D.n_walk && D.comp_top > top) top = D.comp_top;      // (a - node without a mate is written through the complement values)
                if (top >> (8 * w))
                    throw prim::Error(-22, std::string(kWho) + "the image's largest symbol or complement " + std::to_string(top) + " does not fit cell_bytes = " + std::to_string(w));
            }
            cdb_need(nn * sizeof(idx_t) + D.n_walk * sizeof(idx_t) + nn / 8 + nn / 64 * sizeof(idx_t) + 64, "the cells");
        }
        if (uoff) { if (nu) debruijn_copy(D.uoff.p, uoff, nu + 1, "cdebruijn.copy_node_offsets"); else prim::dev_memset(uoff, 0, 8); }
        debruijn_copy(D.uweight.p, weight, nu, "cdebruijn.copy_unitig_weight");
        if (circ && nu) prim::d2d(circ, D.ucirc.p, nu);
        if ((nodes || cells) && nn) {
            DBuf<idx_t> order(nn);
            prim::for_each(nn, CdbOrderFn{D.unitig.p, D.rank.p, D.uoff.p, D.orient.p, order.p}, "cdebruijn.order");
            debruijn_copy(order.p, nodes, nn, "cdebruijn.copy_nodes");
            if (cells) {
                DBuf<RankCell> frc;
                fm_run_cells(*F, frc);
                const CdbStepFn st{KmerStepFn{frc.p, F->key.p, F->slf.p, F->alpha.p}, D.ccode.p, D.cval.p, D.nt};
                const CdbCellSrc src{D.lo.p, D.mate.p};
                with_cell(w, [&](auto c) {
                    typedef decltype(c) cell_t;
#ifdef GRLBWT_PRIM_HIP
                    if (prim::sw().dev_cdebruijn != 'f') {
                        prim::cdb_first_cells<cell_t, idx_t>(nc, nu, k, D.uoff.p, order.p, src, st, (cell_t *)cells);
                        if (D.n_walk) {                          // the - nodes without a mate: k forward steps each, as tickets
                            const u64 nwd = (nn + 63) / 64;
                            DBuf<u64> wbits(nwd);
                            DBuf<idx_t> wrank(nwd + 1), wlist(D.n_walk);
                            DBuf<u64> ctr(2);
                            wbits.zero();
                            prim::bitvector_from_pred(nn, CdbWalkPred{src, order.p}, wbits.p, "cdebruijn.walk_places");
                            (void)prim::exclusive_scan<idx_t>(nwd, PopcIn{wbits.p}, wrank.p, true, "cdebruijn.walk_ranks");
                            prim::for_each_set_bit<idx_t>(nn, wbits.p, wrank.p, CdbWalkListFn{wlist.p}, "cdebruijn.walk_list");
                            (void)prim::walk_tickets(D.n_walk, CdbWalkFn<cell_t>{st, wlist.p, order.p, D.lo.p, D.unitig.p, k, (cell_t *)cells}, ctr.p, "cdebruijn.walks");
                        }
                    } else
#endif
                        prim::for_each(nn, CdbFirstCellFn<cell_t>{st, src, order.p, D.unitig.p, k, (cell_t *)cells}, "cdebruijn.first_cells_plain");
                    if (k > 1) prim::for_each(nu, CdbTailCellsFn<cell_t>{st, src, order.p, D.uoff.p, k, (cell_t *)cells}, "cdebruijn.tail_cells");
                });
                D.cells_forward_steps = nn + D.n_walk * (k - 1) + (k > 1 ? nu * k : 0);
            }
        }
        prim::sync();
    }
    // ---- the strings behind row ranges (functor block "the strings behind row ranges").  docs_create computes what
    // the handle keeps and holds no pointer into the index afterwards.  Everything that can refuse it for its arguments or for
    // memory runs before the first walk; an index without checkpoints keeps no lengths, so there the rows on no string's chain
    // show after the walk, in its step count (fm_sa's rule).  The sort is stable and its rows enter ascending, so every string's
    // rows leave it ascending: the sorted values are LST, neighbours with the same key are PREV.  Peak scratch: the sort's four
    // arrays and a word per walk; the two arrays the sort did not end in are released before PREV is made.
    //   Loops: every walk is bounded by n steps; nothing waits for another thread; the only atomics are the ticket word's.
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kDocsTile = prim::kDocsTile;
#else
    static constexpr u64 kDocsTile = 2048;       // (the serial form has no tiles: the figure the device library reports)
#endif
    static constexpr u32 kDocsOccurrences = 1;
    struct DocsQueryInfo { u64 ranges = 0, range_rows = 0, entries = 0, largest = 0, most = 0; };      // of the last docs_count / docs_list that succeeded
    struct ImageDocs {
        u64 n = 0, k = 0;
        u32 flags = 0;
        u64 scratch_bytes = 0, sort_bits = 0, form = 0, steps = 0;       // of the create
        DBuf<idx_t> da, prev, lst, start;
        mutable DocsQueryInfo q;
        u64 held_bytes() const { return (da.n + prev.n + lst.n + start.n) * sizeof(idx_t); }
    };
    static void docs_create(const FmIndex &F, u32 flags, ImageDocs &D) {
        if (flags & ~kDocsOccurrences) throw prim::Error(-22, "docs: unknown flag bits");
        if (!F.locate) throw prim::Error(-22, "docs: the index was made without the structures for locating");
        const u64 n = F.n, k = F.k;
        const bool occ = (flags & kDocsOccurrences) != 0;
        const u64 tickets = F.checkpoints ? F.walk.m : k;
        D.n = n; D.k = k; D.flags = flags; D.form = F.checkpoints ? 1 : 0;
        D.sort_bits = k > 1 ? (u64)bitlen64(k - 1) : 0;          // ceil(log2 k)
        const u64 held = (2 * n + (occ ? n + k + 1 : 0)) * sizeof(idx_t);
        D.scratch_bytes = (4 * n + tickets) * sizeof(idx_t) + 16;
        if (n >= ((u64)1 << 58) || held + D.scratch_bytes > prim::mem_available())
            throw prim::Error(-12, "docs: the arrays and the sort need " + std::to_string(held + D.scratch_bytes) + " bytes of device memory, more than is free");
        const char *lost = "docs: rows lie on no string's chain: the image is not the BWT of a collection";
        if (F.checkpoints && prim::reduce_sum<u64>(k, SaHeadLenIn{F.smp.p}, "docs.lengths") != n) throw prim::Error(-22, lost);
        D.da.alloc(n);
        {
            constexpr int W = (int)sizeof(idx_t);
            DBuf<idx_t> wsteps(tickets);
            WalkInfo wi;
            const SaWindow win{0, n};
            SaOut<W> so;
            so.p = D.da.p;
            if (F.checkpoints) walk(tickets, SaSegFn<W, 0>{F.lf(), F.sep, F.cp, F.smp.p, win, so, SaOut<0>{}, wsteps.p}, wi, "docs.segments");
            else walk(tickets, SaStringFn<W, 0>{F.lf(), F.sep, n, nullptr, win, so, SaOut<0>{}, wsteps.p}, wi, "docs.strings");
            D.steps = prim::reduce_sum<u64>(tickets, IdxIn64{wsteps.p}, "docs.steps");
        }
        if (!F.checkpoints && D.steps + k != n) throw prim::Error(-22, lost);
        {
            DBuf<idx_t> ka(n), va(n), kb(n), vb(n);
            prim::for_each(n, DocsIotaFn{D.da.p, ka.p, va.p}, "docs.keys");
            const int res = prim::sort_pairs<idx_t, idx_t>(ka.p, va.p, kb.p, vb.p, n, 0, (int)D.sort_bits, "docs.sort");
            DBuf<idx_t> &K = res ? kb : ka, &L = res ? vb : va;
            (res ? ka : kb).release();
            (res ? va : vb).release();
            D.prev.alloc(n);
            prim::for_each(n, DocsPrevFn{K.p, L.p, D.prev.p}, "docs.prev");
            if (occ) {
                D.start.alloc(k + 1);
                prim::for_each(n + 1, DocsStartFn{K.p, n, k, D.start.p}, "docs.starts");
                D.lst = std::move(L);
            }
        }
        prim::sync();
    }
    // docs_count (list = false) and docs_list.  Everything that can refuse the call runs before the first store into an output:
    // the arguments, the ranges, the memory; the flags and their ranks are scratch, and the entries are held against the capacity
    // before the offsets are stored.  n_out is set whenever the count was reached, also when the capacity then refuses the call.
    // The device form of the flags and of the entries is prim::docs_flags / prim::docs_emit (one tile of kDocsTile range rows per
    // workgroup); the stand-in's, and the form they are measured against, bitvector_from_pred and for_each_set_bit with a search
    // in the scanned sizes per range row and per entry.  The counts and the offsets are bit ranks at the ranges' ends either way.
    // Entries with occurrences take the generic form on the device too: the tile kernel with the two searches per entry was
    // measured slower than it (profiles/fm_docs/docs.txt) and does not hold them.
    static void docs_query(const ImageDocs &D, const u64 *lo, const u64 *hi, u64 nr, bool list, u64 *ndocs, u64 *eoff, u64 *str, u64 *frow, u64 *occ,
                           u64 *rng, u64 capacity, u64 &n_out) {
        n_out = 0;
        const std::string who = list ? "docs list" : "docs count";
        if (list && occ && !(D.flags & kDocsOccurrences)) throw prim::Error(-22, who + ": the handle was made without the occurrence lists");
        if (list ? !eoff : (nr && !ndocs)) throw prim::Error(-22, who + ": no output array");
        if (nr && (!lo || !hi)) throw prim::Error(-22, who + ": no ranges");
        DocsQueryInfo qi;
        qi.ranges = nr;
        if (nr == 0) {
            if (list) prim::dev_memset(eoff, 0, 8);
            prim::sync();
            D.q = qi;
            return;
        }
        if (nr >= ((u64)1 << 32)) throw prim::Error(-75, who + ": more ranges than one call takes");
        const u64 bad = prim::reduce_min<u64>(nr, DocsRangeBadIn{lo, hi, D.n}, "docs.ranges");
        if (bad != ~0ull) throw prim::Error(-22, who + ": range " + std::to_string(bad) + " is no range of rows (lo <= hi <= the number of rows)");
        qi.largest = prim::reduce_max<u64>(nr, DocsSpanIn{lo, hi}, "docs.largest_range");
        if (qi.largest && nr > (~0ull >> 2) / qi.largest) throw prim::Error(-75, who + ": more range rows than one call takes");
        if ((nr + 1) * 8 + 64 > prim::mem_available())
            throw prim::Error(-12, who + ": the scanned sizes need " + std::to_string((nr + 1) * 8) + " bytes of device memory, more than is free");
        DBuf<u64> roff(nr + 1);
        const u64 total = qi.range_rows = prim::exclusive_scan<u64>(nr, DocsSpanIn{lo, hi}, roff.p, true, "docs.range_offsets");
#ifdef GRLBWT_PRIM_HIP
        (void)prim::docs_tiles(total, who.c_str());
#endif
        const u64 nw = total / 64 + 2;
        if ((2 * nw + 1) * 8 + 64 > prim::mem_available())
            throw prim::Error(-12, who + ": the flags and their ranks need " + std::to_string((2 * nw + 1) * 8) + " bytes of device memory, more than is free");
        DBuf<u64> words(nw), wrank(nw + 1);
        words.zero();
#ifdef GRLBWT_PRIM_HIP
        const bool tiles = prim::sw().dev_docs_tile != 'f';
        if (tiles) prim::docs_flags<idx_t>(nr, total, roff.p, lo, D.prev.p, words.p);
        else
#endif
            prim::bitvector_from_pred(total, DocsFirstPred{roff.p, lo, D.prev.p, nr}, words.p, "docs.flags_plain");
        const u64 ne = qi.entries = n_out = prim::exclusive_scan<u64>(nw, PopcIn{words.p}, wrank.p, true, "docs.flag_ranks");
        const DocsRank rk{words.p, wrank.p};
        qi.most = prim::reduce_max<u64>(nr, DocsCountIn{roff.p, rk}, "docs.most");
        if (!list) {
            prim::for_each(nr, DocsCountFn{DocsCountIn{roff.p, rk}, ndocs}, "docs.counts");
            prim::sync();
            D.q = qi;
            return;
        }
        if (ne > capacity) throw prim::Error(-22, who + ": " + std::to_string(ne) + " entries, more than the output arrays hold");
        if (ne && !str) throw prim::Error(-22, who + ": no output arrays");
        prim::for_each(nr + 1, DocsOffsetFn{roff.p, rk, eoff}, "docs.entry_offsets");
        if (ne) {
            const DocsOcc oc{D.lst.p, D.start.p};
#ifdef GRLBWT_PRIM_HIP
            if (tiles && !occ) prim::docs_emit<idx_t>(nr, total, nw, ne, roff.p, lo, words.p, wrank.p, D.da.p, str, frow, rng);
            else
#endif
                prim::for_each_set_bit<u64>(total, words.p, wrank.p, DocsEmitFn{roff.p, lo, hi, D.da.p, oc, nr, str, frow, occ, rng}, "docs.emit_plain");
        }
        prim::sync();
        D.q = qi;
    }
    // ---- extract (functor block "extracting text ranges").  Everything that can refuse the call runs before the first
    // store into `out` or `out_off`: the ranges' strings, then the plan -- pieces, cells and steps per range, scanned in scratch --
    // and the capacity.  Then the separators (one lane per range) and the walk, one ticket per piece.
    //   Loops: the binary searches run over the table and the scanned counts; a piece's steps are planned (FmExtractFn); nothing
    //   waits for another thread, and the only atomics are the ticket word's.
    static void fm_string_lengths(const FmIndex &F, u64 *len) {
        if (!F.extract) throw prim::Error(-22, "fm string lengths: the index was made without the structures for extracting");
        prim::for_each(F.k, FmLenOutFn{F.T.p, len}, "fm.string_lengths");
        prim::sync();
    }
    template <class cell_t>
    static void fm_extract_t(const FmIndex &F, const FmExtractPlan &P, u64 nr, const u64 *pscan, const u64 *ooff, u64 pieces, cell_t *out, ExtractInfo &xi) {
        prim::for_each(nr, FmExtractSepFn<cell_t>{P, ooff, out, (cell_t)F.sepval}, "fm.extract_sep");
        WalkInfo wi;
        walk(pieces, FmExtractFn<cell_t>{F.lf(), F.cp, F.xc.p, P, nr, pscan, ooff, out, {F.alpha.p}}, wi, "fm.extract");
        xi.lanes = wi.lanes; xi.refills = wi.refills;
    }
    static u64 fm_extract(const FmIndex &F, const u64 *str, const u64 *beg, const u64 *end, u64 nr, int w, void *out, u64 capacity, u64 *out_off) {
        if (!F.extract) throw prim::Error(-22, "fm extract: the index was made without the structures for extracting");
        check_cell_bytes(w, "fm extract");
        if (w < 8 && (F.maxval >> (8 * w))) throw prim::Error(-22, "fm extract: the image's largest symbol does not fit the cell width");
        ExtractInfo xi;
        xi.ranges = nr;
        if (nr == 0) {
            prim::dev_memset(out_off, 0, 8);
            prim::sync();
            F.xinfo = xi;
            return 0;
        }
        const u64 bad = prim::reduce_min<u64>(nr, FmExtractBadIn{str, F.k}, "fm.extract_strings");
        if (bad != ~0ull) throw prim::Error(-22, "fm extract: range " + std::to_string(bad) + " names a string that is not below the number of strings");
        const FmExtractPlan P{F.T.p, F.xq.p, F.xq.n, str, beg, end};
        DBuf<u64> npiece(nr + 1), ncell(nr + 1), nstep(nr);
        prim::for_each(nr, FmExtractPlanFn{P, npiece.p, ncell.p, nstep.p}, "fm.extract_plan");
        xi.steps = prim::reduce_sum<u64>(nr, CellIn<u64>{nstep.p}, "fm.extract_steps");
        xi.pieces = prim::exclusive_scan<u64>(nr, CellIn<u64>{npiece.p}, npiece.p, true, "fm.extract_pieces");
        xi.cells = prim::exclusive_scan<u64>(nr, CellIn<u64>{ncell.p}, ncell.p, true, "fm.extract_cells");
        if (xi.cells > capacity) throw prim::Error(-22, "fm extract: the ranges hold " + std::to_string(xi.cells) + " cells, more than the output buffer");
        prim::d2d(out_off, ncell.p, (nr + 1) * 8);
        with_cell(w, [&](auto c) {
            typedef decltype(c) cell_t;
            fm_extract_t<cell_t>(F, P, nr, npiece.p, ncell.p, xi.pieces, (cell_t *)out, xi);
        });
        prim::sync();
        F.xinfo = xi;
        return xi.cells;
    }

    // ---- merging two images into the image of "A's strings, then B's" (grlbwt_merge_*; functor block "merging two images";
    // DESIGN.md 4c).  The interleave refinement of Holt and McMillan: z starts as 0^nA 1^nB; a round writes every row's flag where
    // a stable sort of the rows by their symbol puts it and resets the separator's bucket to 0^kA 1^kB (the terminators are
    // ordered by the strings' numbers); the rounds end with the one that changes nothing.
    struct ImageMerge {
        u64 na = 0, nb = 0, ka = 0, kb = 0, sigma = 0, sepval = 0;
        u64 rounds = 0, rows_changed = 0, n_runs = 0, out_bytes = 0, sb = 0, fb = 0, scratch_bytes = 0;
        DBuf<u8> ra, rb, z;       // rank byte per row of A and of B (16 bytes of padding behind each), the converged interleave
        DBuf<u64> alpha;          // rank -> symbol value
        u64 held_bytes() const { return ra.n + rb.n + z.n + alpha.n * 8; }
    };
#ifdef GRLBWT_PRIM_HIP
    static constexpr u64 kMergeTile = prim::kMgTile;
#else
    static constexpr u64 kMergeTile = 4096;      // (the serial form has no tiles: the figure the device library reports)
#endif
    static constexpr u64 kMergeSigmaMax = 256;
    // the non-empty records of an image: their symbols as 64-bit values and their lengths
    static u64 merge_load_runs(const void *dev_image, u64 image_bytes, const char *which, DBuf<u64> &val, DBuf<idx_t> &len) {
        const ImageHeader h = image_header(dev_image, image_bytes);
        if (h.R == 0) throw prim::Error(-22, std::string("merge: image ") + which + " has no record");
        val.alloc(h.R); len.alloc(h.R);
        prim::for_each(h.R, UnpackRunsFn<u64>{h.recs(dev_image), val.p, len.p}, "merge.unpack");
        const u64 R = drop_empty_runs(val, len, h.R, "merge");
        if (R == 0) throw prim::Error(-22, std::string("merge: image ") + which + " describes no symbol");
        return R;
    }
    // rank byte per row of one image: out[0, n) (allocated with the padding the round kernels read over); returns n
    static u64 merge_expand(const u32 *rrank, const idx_t *rlen, u64 R, DBuf<u8> &out) {
        DBuf<idx_t> rpos(R + 1);
        const u64 n = (u64)prim::exclusive_scan<idx_t>(R, IdxIn<idx_t>{rlen}, rpos.p, true, "merge.positions");
        RankBits rb;
        build_rankbits(rb, rpos.p, R, n + 1, "merge.runbits");
        out.alloc(n + 16);
        prim::for_each(n, MgExpandFn{rrank, rb.words.p, rb.base.p, out.p}, "merge.expand");
        return n;
    }
    // the interleave as a bit-vector with ranks, and the run heads of the merged sequence read through it
    struct MergeHeads { RankBits zb; DBuf<u64> hw; DBuf<idx_t> hb; u64 R = 0; };
    static u64 merge_heads_bytes(u64 n) { return (n / 64 + 3) * 2 * (8 + sizeof(idx_t)); }
    static void merge_bits(const u8 *z, u64 n, RankBits &zb) {
        const u64 nw = n / 64 + 2;
        zb.words.alloc(nw); zb.base.alloc(nw + 1);
        zb.words.zero();
        prim::bitvector_from_pred(n, MgFlagPred{z}, zb.words.p, "merge.bits");
        prim::exclusive_scan_nosync<idx_t>(nw, PopcIn{zb.words.p}, zb.base.p, true, "merge.bit_ranks");
    }
    static MgSym merge_sym(const ImageMerge &M, const RankBits &zb) { return MgSym{M.ra.p, M.rb.p, zb.words.p, zb.base.p}; }
    static void merge_heads(const ImageMerge &M, MergeHeads &H) {
        const u64 n = M.na + M.nb, nw = n / 64 + 2;
        merge_bits(M.z.p, n, H.zb);
        H.hw.alloc(nw); H.hb.alloc(nw + 1);
        H.hw.zero();
        prim::bitvector_from_pred(n, MgHeadPred{merge_sym(M, H.zb)}, H.hw.p, "merge.heads");
        H.R = (u64)prim::exclusive_scan<idx_t>(nw, PopcIn{H.hw.p}, H.hb.p, true, "merge.head_ranks");
    }
    // One refinement round without the separator rule, and the test that ends the rounds.  changed(): the rows at which the
    // interleave `cur` differs from `prev`, the one before it (null: 0) -- the device form takes the A-rows per tile of `cur` in
    // the same pass, so it comes first; step(): oth = the flags of cur where a stable sort of the rows by their symbol puts them.
    // The device form is prim::MgRound (three kernels, the symbols read from two contiguous slices per tile); the serial form
    // goes through the generic primitives: the merged symbols gathered as keys, a stable sort of (key, flag).
    struct MergeRound {
        u64 n = 0;
        bool by_sort = !prim::kIsDevice;
        static u64 sort_scratch_bytes(u64 n_) { return 3 * n_ + (n_ / 64 + 3) * (8 + sizeof(idx_t)) + (n_ / 4096 + 1) * 256 * 12; }
        u64 changed_by_sum(const u8 *cur, const u8 *prev) { return prev ? prim::reduce_sum<u64>(n, MgDiffIn{cur, prev}, "merge.changed") : 0; }
        void step_by_sort(const u8 *ra, const u8 *rb, const u8 *cur, u8 *oth) {
            RankBits zb;
            merge_bits(cur, n, zb);
            DBuf<u8> ka(n), kb(n), v2(n);
            prim::for_each(n, MgKeyFn{MgSym{ra, rb, zb.words.p, zb.base.p}, ka.p}, "merge.keys");
            d2d_copy(oth, cur, n);
            const int res = prim::sort_pairs<u8, u8>(ka.p, oth, kb.p, v2.p, n, 0, 8, "merge.sort");
            if (res) d2d_copy(oth, v2.p, n);
        }
#ifdef GRLBWT_PRIM_HIP
        // (GRLBWT_MERGE_ROUND=sort: the generic form on the device too -- the baseline the fused kernels are measured against)
        prim::MgRound<idx_t> W;
        static u64 scratch_bytes(u64 n_) { return prim::sw().merge_round == 's' ? sort_scratch_bytes(n_) : prim::MgRound<idx_t>::scratch_bytes(n_); }
        void alloc(u64 n_) { n = n_; by_sort = prim::sw().merge_round == 's'; if (!by_sort) W.alloc(n_); }
        void release() { W.release(); }
        u64 changed(const u8 *cur, const u8 *prev, u64 na) {
            if (by_sort) return changed_by_sum(cur, prev);
            u64 a_rows = 0;
            const u64 c = W.count(cur, prev, &a_rows);
            if (a_rows != na) throw prim::Error(-71, "merge: a round lost rows of A");
            return c;
        }
        void step(const u8 *ra, const u8 *rb, const u8 *cur, u8 *oth) { if (by_sort) step_by_sort(ra, rb, cur, oth); else W.scatter(cur, ra, rb, oth); }
#else
        static u64 scratch_bytes(u64 n_) { return sort_scratch_bytes(n_); }
        void alloc(u64 n_) { n = n_; }
        void release() {}
        u64 changed(const u8 *cur, const u8 *prev, u64) { return changed_by_sum(cur, prev); }
        void step(const u8 *ra, const u8 *rb, const u8 *cur, u8 *oth) { step_by_sort(ra, rb, cur, oth); }
#endif
    };
    // device milliseconds the profile table holds under a kernel name (0 while the profile is off)
    static double merge_prof_ms(const char *name) {
        auto it = prim::rt().prof.find(name);
        return it == prim::rt().prof.end() ? 0.0 : (double)it->second.ms;
    }
    // The header rule of an image and its records, shared by what writes an image from runs (merge, select).  sb comes from the
    // largest symbol + 4, fb from `longest`: the largest total of one symbol (cells of one byte) or the number of symbols.
    static void image_widths(u64 max_sym, u64 longest, u64 &sb, u64 &fb) {
        sb = (bitlen64(max_sym + 4) + 7) / 8;
        fb = (bitlen64(longest) + 7) / 8;
    }
    static void emit_records(const u32 *sym, RunLen len, u64 R, u32 sb, u32 fb, const u64 *alpha, u8 *out, const char *name) {
        u8 hdr[16] = {0};
        hdr[0] = (u8)sb; hdr[8] = (u8)fb;
        prim::h2d(out, hdr, 16);
        if (sb + fb <= 8 && fb < 8) prim::pack_records(R, RunRecordFn{sym, len, sb, alpha}, sb + fb, out + 16, name);
        else prim::for_each(R, PackRunsFn{sym, len, sb, fb, out, 16u, alpha}, name);
    }
    static void merge_create(const void *img_a, u64 bytes_a, const void *img_b, u64 bytes_b, int cell_bytes, u64 max_rounds, ImageMerge &M) {
        check_cell_bytes(cell_bytes, "merge");
        // ---- load: the records of both images, the union of their symbol values, one rank byte per row
        DBuf<u64> va, vb;
        DBuf<idx_t> la, lb;
        const u64 Ra = merge_load_runs(img_a, bytes_a, "A", va, la), Rb = merge_load_runs(img_b, bytes_b, "B", vb, lb);
        DBuf<u64> cat(Ra + Rb);
        d2d_copy(cat.p, va.p, Ra);
        d2d_copy(cat.p + Ra, vb.p, Rb);
        va.release(); vb.release();
        const u64 mx = prim::reduce_max<u64>(Ra + Rb, CellIn<u64>{cat.p}, "merge.max_sym");
        if (cell_bytes < 8 && (mx >> (8 * cell_bytes))) throw prim::Error(-22, "merge: the largest symbol (" + std::to_string(mx) + ") does not fit the cell width");
        DBuf<u32> ranks(Ra + Rb);
        M.sigma = alphabet_compact<u64>(cat.p, Ra + Rb, mx, ranks.p, M.alpha);
        cat.release();
        if (M.sigma > kMergeSigmaMax)
            throw prim::Error(-75, "merge: the two images hold " + std::to_string(M.sigma) + " distinct symbols together, more than the 256 a round sorts by");
        const std::vector<u64> alpha = M.alpha.to_host(M.sigma);
        const u32 sep_a = prim::reduce_min<u32>(Ra, PtrU32In{ranks.p}, "merge.sep_a"), sep_b = prim::reduce_min<u32>(Rb, PtrU32In{ranks.p + Ra}, "merge.sep_b");
        if (sep_a != sep_b)
            throw prim::Error(-22, "merge: the smallest symbols of the two images differ (" + std::to_string(alpha[sep_a]) + " in A, " + std::to_string(alpha[sep_b]) +
                                       " in B): they are not collections with one separator");
        M.sepval = alpha[0];
        M.na = merge_expand(ranks.p, la.p, Ra, M.ra);
        M.nb = merge_expand(ranks.p + Ra, lb.p, Rb, M.rb);
        ranks.release(); la.release(); lb.release();
        const u64 n = M.na + M.nb;
        u64 ha[256], hb[256];
        prim::byte_histogram(M.ra.p, M.na, ha);
        prim::byte_histogram(M.rb.p, M.nb, hb);
        M.ka = ha[0]; M.kb = hb[0];
        u64 F = n;
        if (cell_bytes == 1) { F = 0; for (int i = 0; i < 256; i++) if (ha[i] + hb[i] > F) F = ha[i] + hb[i]; }
        image_widths(mx, F, M.sb, M.fb);
        // ---- the rounds.  Scratch: the second interleave buffer, the tile tables, and what the run heads take afterwards
        const u64 round_scratch = MergeRound::scratch_bytes(n);
        M.scratch_bytes = (n + 16) + std::max(round_scratch, merge_heads_bytes(n));
        if (M.scratch_bytes + (n + 16) > prim::mem_available())
            throw prim::Error(-12, "merge: the rounds need " + std::to_string(M.scratch_bytes + n + 16) + " bytes of device memory, more than is free");
        DBuf<u8> z0(n + 16), z1(n + 16);
        u8 *cur = z0.p, *oth = z1.p;
        prim::for_each(n, MgSplitFn{cur, M.na}, "merge.first");
        const u64 cap = max_rounds ? max_rounds : n + 2, k = M.ka + M.kb;
        bool converged = false;
        MergeRound W;
        W.alloc(n);
        prim::rt().tag = -1; prim::rt().phase = 0;
        const char *kinds[6] = {"merge.counts", "merge.hist", "merge.scatter", "merge.changed", "merge.keys", "merge.sort.scatter"};
        double seen[6] = {0, 0, 0, 0, 0, 0};
        for (;;) {
            const u64 changed = W.changed(cur, M.rounds ? oth : nullptr, M.na);
            if (prim::rt().profile) {
                // the per-round log (grlbwt_profile_enable): the kernels of the round just done and the pass that found what it changed
                double ms[6];
                for (int i = 0; i < 6; i++) { const double t = merge_prof_ms(kinds[i]); ms[i] = t - seen[i]; seen[i] = t; }
                if (M.rounds)
                    fprintf(stderr, "[grlbwt] merge round %llu: rows changed %llu; ms: counts %.3f hist %.3f scatter %.3f (sort form: changed %.3f keys %.3f sort scatter %.3f)\n",
                            (unsigned long long)M.rounds, (unsigned long long)changed, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
            }
            if (M.rounds) {
                M.rows_changed += changed;
                if (changed == 0) { converged = true; break; }
            }
            if (M.rounds == cap) break;
            W.step(M.ra.p, M.rb.p, cur, oth);
            prim::for_each(k, MgSplitFn{oth, M.ka}, "merge.separators");
            std::swap(cur, oth);
            M.rounds++;
        }
        if (!converged)
            throw prim::Error(-22, "merge: not converged after " + std::to_string(M.rounds) + " rounds (max_rounds); the rounds needed are about the longest prefix a suffix of A "
                                   "shares with a suffix of B -- the per-string cost model of grlbwt_fm_locate without checkpoints: fine for reads, hopeless for chromosomes");
        W.release();
        if (cur == z0.p) { M.z = std::move(z0); z1.release(); } else { M.z = std::move(z1); z0.release(); }
        MergeHeads H;
        merge_heads(M, H);
        M.n_runs = H.R;
        M.out_bytes = 16 + H.R * (M.sb + M.fb);
        prim::sync();
    }
    static void merge_emit(const ImageMerge &M, u8 *out, u64 capacity) {
        if (capacity < M.out_bytes) throw prim::Error(-22, "merge: output buffer too small (" + std::to_string(M.out_bytes) + " bytes needed)");
        const u64 n = M.na + M.nb;
        MergeHeads H;
        merge_heads(M, H);
        if (H.R != M.n_runs) throw prim::Error(-71, "merge: the run heads changed since the merge was made");
        const u64 R = H.R;
        DBuf<u32> sym(R);
        DBuf<idx_t> start(R + 1);
        prim::for_each_set_bit<idx_t>(n, H.hw.p, H.hb.p, MgHeadFn{merge_sym(M, H.zb), sym.p, start.p}, "merge.runs");
        const idx_t total = (idx_t)n;
        prim::h2d(start.p + R, &total, sizeof(total));
        emit_records(sym.p, RunLen{nullptr, start.p}, R, (u32)M.sb, (u32)M.fb, M.alpha.p, out, "merge.pack");
        prim::sync();
    }
    static void merge_interleave(const ImageMerge &M, u64 *dev_bits) {
        prim::bitvector_from_pred(M.na + M.nb, MgFlagPred{M.z.p}, dev_bits, "merge.interleave");
        prim::sync();
    }

    // ---- removing or keeping chosen strings of an image (grlbwt_select_*; functor block "removing or keeping chosen strings";
    // DESIGN.md 4e).  The list becomes a k-bit set; the chains of the listed strings are marked in an n-bit vector, per string or
    // through checkpointed segments; a rank over the marked bits gives every run its new length; empty runs go, equal neighbours
    // are joined.  The handle keeps the new runs, the values of a compacted alphabet and the marked bits.
    //   Loops: a string's walk is bounded by n steps, a segment's by seglen[c] + 1, the pointer jumping by ceil(log2 m) rounds;
    //   nothing waits for another thread; the atomics are the ticket word's and the ORs into the two bit-vectors.
    struct ImageSelect {
        u64 n_in = 0, k_in = 0, R_in = 0, n_listed = 0, rows_marked = 0, longest_walk = 0;
        u64 n_out = 0, k_out = 0, R_out = 0, out_bytes = 0, sb = 0, fb = 0, sepval = 0, flags = 0;
        u64 lanes = 0, refills = 0, sample_bits = 0, n_checkpoints = 0, jump_rounds = 0, scratch_bytes = 0;
        DBuf<u32> sym;            // the runs of the output: symbols (ranks where alpha is set) and lengths
        DBuf<idx_t> len;
        DBuf<u64> alpha;          // rank -> symbol value (null: the symbols are the values)
        DBuf<u64> marked;         // bit p: row p of the input lies on a listed string's chain
        u64 held_bytes() const { return sym.n * 4 + len.n * sizeof(idx_t) + alpha.n * 8 + marked.n * 8; }
    };
    static void select_create(const void *dev_image, u64 image_bytes, int cell_bytes, const u64 *ids, u64 n_ids, bool keep, bool checkpoints, int sample_bits,
                              ImageSelect &S) {
        check_cell_bytes(cell_bytes, "select");
        if (!checkpoints && sample_bits) throw prim::Error(-22, "select: sample_bits needs the checkpoint flag");
        const int b = checkpoints ? sample_bits_of(sample_bits) : 0;
        const ImageHeader h = image_header(dev_image, image_bytes);
        if (h.R == 0) throw prim::Error(-22, "select: the image has no record");
        WideSyms W;
        image_symbols(h.recs(dev_image), h.R, cell_bytes, W, "select");
        RunIndex X;
        run_index_load(h.recs(dev_image), h.R, W, X);
        W.ranks.release();
        const u64 R = X.R, n = X.n, k = X.k;
        if (R == 0) throw prim::Error(-22, "select: the image describes no symbol");
        const u32 sep = X.sep;
        S.n_in = n; S.k_in = k; S.R_in = R;
        S.sepval = W.alpha.p ? W.alpha.get(sep) : (u64)sep;
        // ---- the list as a set, its distinct entries in ascending order as the tickets
        if (n_ids) {
            const u64 bad = prim::reduce_min<u64>(n_ids, FmExtractBadIn{ids, k}, "select.list_check");
            if (bad != ~0ull) {
                u64 v = 0;
                prim::d2h(&v, ids + bad, 8);
                throw prim::Error(-22, "select: entry " + std::to_string(bad) + " of the list (" + std::to_string(v) + ") is not below the number of strings (" +
                                           std::to_string(k) + ")");
            }
        }
        const u64 lw = k / 64 + 2;
        DBuf<u64> list(lw);
        DBuf<idx_t> lbase(lw + 1);
        list.zero();
        prim::for_each(n_ids, SelListFn{ids, list.p}, "select.list");
        const u64 nl = (u64)prim::exclusive_scan<idx_t>(lw, PopcIn{list.p}, lbase.p, true, "select.list_ranks");
        S.n_listed = nl;
        S.k_out = keep ? nl : k - nl;
        if (S.k_out == 0)
            throw prim::Error(-22, keep ? "select: the keep flag with an empty list leaves no string" : "select: every string is listed, the result would hold no string");
        // ---- memory, before the first walk: the run index and its sort, the two bit-vectors with their ranks, the tickets, the
        // checkpoint ranking's arrays, the rewrite's scan
        const u64 words = (n + 1) / 64 + 2, mw = n / 64 + 2;
        const u64 m = checkpoints ? Checkpoints{n, k, (u32)b}.count() : 0;
        u64 need = words * (sizeof(RankCell) + 8 + sizeof(idx_t)) + R * (sizeof(RunRec) + 3 * (4 + sizeof(idx_t))) + lw * (8 + sizeof(idx_t)) +
                   mw * (8 + sizeof(idx_t)) + 2 * nl * sizeof(idx_t);
        if (checkpoints) need += (6 * m + 2 * k + 1) * sizeof(idx_t) + k * 8;
        S.scratch_bytes = need;
        if (need > prim::mem_available())
            throw prim::Error(-12, "select: the structures need " + std::to_string(need) + " bytes of device memory, more than is free");
        DBuf<idx_t> tick(nl);
        prim::for_each_set_bit<idx_t>(k, list.p, lbase.p, SelTicketFn{tick.p}, "select.tickets");
        lbase.release();
        run_index_lf(X, true, false, true);
        // ---- marking
        S.marked.alloc(mw);
        S.marked.zero();
        u64 listed_len = 0;
        WalkInfo wi;
        if (!checkpoints) {
            DBuf<idx_t> steps(nl);
            DBuf<u32> bad(1);
            bad.zero();
            walk(nl, SelMarkFn{X.lf(), sep, n, tick.p, S.marked.p, steps.p, bad.p}, wi, "select.mark");
            if (nl && bad.get(0)) throw prim::Error(-22, "select: a string's walk met no separator in n steps: not the BWT of a collection");
            listed_len = prim::reduce_sum<u64>(nl, IdxIn64{steps.p}, "select.steps");
            S.longest_walk = prim::reduce_max<u64>(nl, IdxIn64{steps.p}, "select.longest");
        } else {
            CpRank C;
            lf_checkpoints(X.lf(), n, k, sep, b, -22, C, wi);
            walk(m, SelMarkCpFn{X.lf(), sep, C.cp, C.head.p, C.seglen.p, list.p, S.marked.p}, wi, "select.mark_cp");
            listed_len = prim::reduce_sum<u64>(nl, SelListedLenIn{tick.p, C.slen.p}, "select.steps");
            S.longest_walk = prim::reduce_max<u64>(m, SelSegStepsIn{C.head.p, C.seglen.p, list.p}, "select.longest");
            S.sample_bits = (u64)b; S.n_checkpoints = m; S.jump_rounds = wi.jump_rounds;
        }
        S.lanes = wi.lanes; S.refills = wi.refills;
        X.rc.release(); X.rec.release(); tick.release(); list.release();
        // ---- the rewrite: ranks over the marked words, the new length of every run, maximal runs
        {
            DBuf<idx_t> mbase(mw + 1);
            S.rows_marked = (u64)prim::exclusive_scan<idx_t>(mw, PopcIn{S.marked.p}, mbase.p, true, "select.ranks");
            if (S.rows_marked != listed_len) throw prim::Error(-71, "select: the rows marked do not add up to the lengths of the listed strings");
            prim::for_each(R, SelRunLenFn{X.rpos.p, S.marked.p, mbase.p, keep, X.rlen.p}, "select.run_lengths");
        }
        X.rpos.release();
        const u64 R2 = drop_empty_runs(X.rsym, X.rlen, R);
        Runs out = merge_runs(X.rsym.p, X.rlen.p, R2);
        X.rsym.release(); X.rlen.release(); out.pos.release();
        S.R_out = out.R; S.n_out = out.n;
        if (S.n_out != (keep ? S.rows_marked : n - S.rows_marked)) throw prim::Error(-71, "select: the rewritten runs do not add up");
        if (prim::reduce_sum<u64>(out.R, SepLenIn{out.sym.p, out.len.p, sep}, "select.separators") != S.k_out)
            throw prim::Error(-71, "select: the rewritten runs do not hold one separator per remaining string");
        // ---- the header: the largest remaining symbol; the largest total of one symbol (cells of one byte) or the length
        const u32 mxr = prim::reduce_max<u32>(out.R, PtrU32In{out.sym.p}, "select.max_sym");
        const u64 mx = W.alpha.p ? W.alpha.get(mxr) : (u64)mxr;
        u64 F = S.n_out;
        if (cell_bytes == 1) {
            DBuf<u64> bins(256);
            bins.zero();
            prim::for_each_agg(out.R, RunSymFn{out.sym.p}, BinAddFn{bins.p}, true, "select.runs_per_symbol");
            const std::vector<u64> hb = bins.to_host(256);
            F = 0;
            for (u32 c = 0; c < 256; c++)
                if (hb[c]) F = std::max(F, prim::reduce_sum<u64>(out.R, SepLenIn{out.sym.p, out.len.p, c}, "select.symbol_total"));
        }
        image_widths(mx, F, S.sb, S.fb);
        S.out_bytes = 16 + S.R_out * (S.sb + S.fb);
        S.sym = std::move(out.sym); S.len = std::move(out.len);
        S.alpha = std::move(W.alpha);
        prim::sync();
    }
    static void select_emit(const ImageSelect &S, u8 *out, u64 capacity) {
        if (capacity < S.out_bytes) throw prim::Error(-22, "select: output buffer too small (" + std::to_string(S.out_bytes) + " bytes needed)");
        emit_records(S.sym.p, RunLen{S.len.p, nullptr}, S.R_out, (u32)S.sb, (u32)S.fb, S.alpha.p, out, "select.pack");
        prim::sync();
    }
    static void select_rows(const ImageSelect &S, u64 *dev_bits) {
        prim::d2d(dev_bits, S.marked.p, (S.n_in + 63) / 64 * 8);
        prim::sync();
    }

    // number of symbols an image describes, summed in 64 bits whatever the index width of the caller
    static u64 image_total_symbols(const void *dev_image, u64 image_bytes) {
        ImageHeader h = image_header(dev_image, image_bytes);
        return prim::reduce_sum<u64>(h.R, ImageLenIn{h.recs(dev_image)}, "image.total");
    }
    // grl2plain (scripts/grl2plain.cpp): the plain BWT, one byte per symbol; null_char >= 0 replaces symbol 0
    static u64 image_plain(const void *dev_image, u64 image_bytes, u8 *dev_out, u64 capacity, int null_char) {
        ImageHeader h = image_header(dev_image, image_bytes);
        DBuf<u32> rsym(h.R);
        DBuf<idx_t> rlen(h.R), rpos(h.R + 1);
        prim::for_each(h.R, UnpackRunsFn<u32>{h.recs(dev_image), rsym.p, rlen.p}, "plain.unpack");
        prim::for_each(h.R, PlainSymFn{h.recs(dev_image), null_char, rsym.p}, "plain.bytes");
        const u64 R = drop_empty_runs(rsym, rlen, h.R);
        u64 n = (u64)prim::exclusive_scan<idx_t>(R, IdxIn<idx_t>{rlen.p}, rpos.p, true, "plain.positions");
        if (n > capacity) throw prim::Error(-22, "grl2plain: output buffer too small");
        RankBits rb;
        build_rankbits(rb, rpos.p, R, n + 1, "plain.runbits");
        prim::for_each(n, PlainRunsFn{rsym.p, rb.words.p, rb.base.p, dev_out}, "plain.expand");
        prim::sync();
        return n;
    }
    // grlbwt2rle (scripts/grlbwt2rle.cpp): the two RLE arrays
    static u64 image_rle(const void *dev_image, u64 image_bytes, u8 *dev_syms, u32 *dev_lens, u64 capacity_runs) {
        ImageHeader h = image_header(dev_image, image_bytes);
        if (h.R > capacity_runs) throw prim::Error(-22, "grlbwt2rle: output buffers too small");
        DBuf<u32> rsym(h.R);
        DBuf<idx_t> rlen(h.R);
        prim::for_each(h.R, UnpackRunsFn<u32>{h.recs(dev_image), rsym.p, rlen.p}, "rle.unpack");
        prim::for_each(h.R, RleExportFn{rsym.p, rlen.p, dev_syms, dev_lens}, "rle.export");
        prim::sync();
        return h.R;
    }
    // bwt_stats (scripts/bwt_stats.cpp:18-98), byte alphabets (the reference indexes 256-entry tables by the symbol)
    struct ImageStats {
        u64 n_runs, sigma, text_size, min_run, max_run, fit1, fit2, fit3;
        u64 runs_of[256], freq_of[256];
        u64 deciles[9];
        u64 non_maximal;
    };
    static void image_stats(const void *dev_image, u64 image_bytes, ImageStats &st) {
        ImageHeader h = image_header(dev_image, image_bytes);
        if (h.sb != 1) throw prim::Error(-22, "bwt_stats: byte alphabets only (sb == 1)");
        if (h.R == 0) throw prim::Error(-22, "bwt_stats: empty BWT");
        const u64 R = h.R;
        DBuf<u32> rsym(R);
        DBuf<idx_t> rlen(R);
        prim::for_each(R, UnpackRunsFn<u32>{h.recs(dev_image), rsym.p, rlen.p}, "stats.unpack");
        st.n_runs = R;
        st.min_run = prim::reduce_min<u64>(R, IdxIn64{rlen.p}, "stats.min_run");
        st.max_run = prim::reduce_max<u64>(R, IdxIn64{rlen.p}, "stats.max_run");
        st.text_size = prim::reduce_sum<u64>(R, IdxIn64{rlen.p}, "stats.text_size");
        st.fit1 = prim::reduce_sum<u64>(R, LenFitIn{rlen.p, 1}, "stats.fit1");
        st.fit2 = prim::reduce_sum<u64>(R, LenFitIn{rlen.p, 2}, "stats.fit2");
        st.fit3 = R - st.fit1 - st.fit2;
        st.non_maximal = R - prim::reduce_sum<u64>(R, SymHeadIn64{rsym.p}, "stats.maximal");
        DBuf<u64> bins(256);
        bins.zero();
        prim::for_each_agg(R, RunSymFn{rsym.p}, BinAddFn{bins.p}, true, "stats.runs_per_symbol");
        std::vector<u64> hb = bins.to_host(256);
        st.sigma = 0;
        for (int c = 0; c < 256; c++) {
            st.runs_of[c] = hb[c];
            st.freq_of[c] = hb[c] ? prim::reduce_sum<u64>(R, SepLenIn{rsym.p, rlen.p, (u32)c}, "stats.freq") : 0;
            if ((hb[c] & 0xFFu) != 0) st.sigma++;       // the reference iterates the table as unsigned char (:57-62)
        }
        // deciles of the sorted run lengths (uint32 like the reference's vector), index ceil(R * k/10) with the
        // reference's accumulated double (:83-89); an index past the end (R < 10) is clamped to the last run
        DBuf<u32> ka(R), kb(R), va(R), vb(R);
        prim::for_each(R, LenKeyFn{rlen.p, ka.p, va.p}, "stats.len_keys");
        int res = prim::sort_pairs<u32, u32>(ka.p, va.p, kb.p, vb.p, R, 0, 32, "stats.sort");
        const DBuf<u32> &sorted = res ? kb : ka;
        double l = (double)R, prop = 0.1;
        for (int i = 0; i < 9; i++) {
            u64 q = (u64)std::ceil(l * prop);
            if (q >= R) q = R - 1;
            st.deciles[i] = sorted.get(q);
            prop += 0.1;
        }
    }

    // split_runs (scripts/split_runs.cpp): re-encode an image with run lengths of at most 2^bits - 1 and, for
    // block_size > 0, no run crossing a multiple of block_size; run-length field of ceil(bits/8) bytes.  block_size 0
    // = no partition (what the reference's usage text promises; its own code asserts there).
    struct SplitInfo { u64 runs_before, runs_after, overflow_splits, block_splits, n_syms, out_bytes; };
    static SplitInfo image_split_runs(const void *dev_image, u64 image_bytes, int bits, u64 block_size, u8 *dev_out, u64 capacity_bytes) {
        ImageHeader h = image_header(dev_image, image_bytes);
        if (bits < 1 || bits > 63) throw prim::Error(-22, "split_runs: bits must be in [1, 63]");
        const u64 L = (1ull << bits) - 1, B = block_size, R = h.R;
        const u32 fb2 = (u32)((bits + 7) / 8);
        // (the pieces carry their symbol in 32 bits: a wider one is refused, not cut)
        if (h.sb > 4 && prim::reduce_max<u64>(R, ImageSymIn{h.recs(dev_image)}, "split.max_sym") >> 32)
            throw prim::Error(-22, "split_runs: symbols >= 2^32 are not supported");
        DBuf<u32> rsym(R);
        DBuf<idx_t> rlen(R), rpos(R + 1), jbase(R + 1);
        prim::for_each(R, UnpackRunsFn<u32>{h.recs(dev_image), rsym.p, rlen.p}, "split.unpack");
        const u64 n = (u64)prim::exclusive_scan<idx_t>(R, IdxIn<idx_t>{rlen.p}, rpos.p, true, "split.positions");
        const u64 J = (u64)prim::exclusive_scan<idx_t>(R, PieceCountFn{rlen.p, L}, jbase.p, true, "split.pieces");
        const u64 cuts = (B && n > 0) ? (n - 1) / B : 0;
        SplitInfo si{R, J + cuts, J - R, cuts, n, 16 + (J + cuts) * (u64)(h.sb + fb2)};
        if (si.out_bytes > capacity_bytes) throw prim::Error(-22, "split_runs: output buffer too small");
        RankBits jb;
        build_rankbits(jb, jbase.p, R, J + 1, "split.piecebits");
        DBuf<u32> osym(si.runs_after);
        DBuf<idx_t> olen(si.runs_after);
        prim::for_each(J, SplitRunsFn{rsym.p, rlen.p, rpos.p, jbase.p, jb.words.p, jb.base.p, L, B, osym.p, olen.p}, "split.emit");
        u8 hdr[16] = {0};
        for (int i = 0; i < 8; i++) { hdr[i] = (u8)(h.sb >> (8 * i)); hdr[8 + i] = (u8)((u64)fb2 >> (8 * i)); }
        prim::h2d(dev_out, hdr, 16);
        prim::for_each(si.runs_after, PackRunsFn{osym.p, RunLen{olen.p, nullptr}, (u32)h.sb, fb2, dev_out, 16u}, "split.pack");
        prim::sync();
        return si;
    }
};

}   // namespace GRL_NS

#endif   // once per index width
