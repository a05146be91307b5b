// capi_impl.hpp -- extern "C" layer of include/grlbwt_hip.h over the two index-width
// instantiations of the engine (grl32 / grl64).  Included by engine_hip.hip.
#include "../../include/grlbwt_hip.h"

#include <fcntl.h>
#include <zlib.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>


// an FM index (grlbwt_fm_create): one of the two index widths; its buffers come from the context's pool
struct grlbwt_fm {
    uint32_t flags = 0;
    std::unique_ptr<grl32::Image::FmIndex> f32;
    std::unique_ptr<grl64::Image::FmIndex> f64;
};

// a merge of two images (grlbwt_merge_create): the converged interleave, the two rank sequences and the alphabet
struct grlbwt_merge {
    std::unique_ptr<grl32::Image::ImageMerge> m32;
    std::unique_ptr<grl64::Image::ImageMerge> m64;
};

// a selection of strings (grlbwt_select_create): the rewritten runs, the alphabet and the marked rows
struct grlbwt_select {
    std::unique_ptr<grl32::Image::ImageSelect> s32;
    std::unique_ptr<grl64::Image::ImageSelect> s64;
};

// the strings behind row ranges (grlbwt_docs_create): the document array and what the queries read beside it
struct grlbwt_docs {
    std::unique_ptr<grl32::Image::ImageDocs> d32;
    std::unique_ptr<grl64::Image::ImageDocs> d64;
};

// a compacted de Bruijn graph (grlbwt_debruijn_create): the nodes, the in-edges and the unitigs
struct grlbwt_debruijn {
    std::unique_ptr<grl32::Image::ImageDeBruijn> g32;
    std::unique_ptr<grl64::Image::ImageDeBruijn> g64;
};

// a strand-merged compacted de Bruijn graph (grlbwt_cdebruijn_create): the nodes, the half-edges of their ends and the unitigs
struct grlbwt_cdebruijn {
    std::unique_ptr<grl32::Image::ImageCDeBruijn> g32;
    std::unique_ptr<grl64::Image::ImageCDeBruijn> g64;
};

struct grlbwt_ctx {
    uint32_t flags = 0;
    int device = 0;
    std::unique_ptr<grl32::Engine> e32;
    std::unique_ptr<grl64::Engine> e64;
    mutable std::string err;           // grlbwt_last_error: the message of the last call that failed (const calls refuse too)
    std::vector<grlbwt_fm *> fms;      // the indexes still alive: released with the context
    std::vector<grlbwt_merge *> merges;      // and the merges
    std::vector<grlbwt_select *> selects;    // and the selections
    std::vector<grlbwt_docs *> docs;         // and the document handles
    std::vector<grlbwt_debruijn *> graphs;   // and the de Bruijn graphs
    std::vector<grlbwt_cdebruijn *> cgraphs; // and the strand-merged ones
};

namespace {

// Every C-API call that runs engine or primitive work goes through here: it takes the switch snapshot the call runs with.
template <class Fn>
int guarded(grlbwt_ctx *ctx, Fn fn) {
    prim::take_switches();
    try {
        fn();
        return GRLBWT_OK;
    } catch (const prim::Error &e) {
        if (ctx) ctx->err = e.what();
        return e.code;
    } catch (const std::bad_alloc &) {
        if (ctx) ctx->err = "host allocation failed";
        return GRLBWT_ENOMEM;
    } catch (const std::exception &e) {
        if (ctx) ctx->err = e.what();
        return GRLBWT_EINTERNAL;
    }
}

template <class E>
void fill_round(const E &e, int r, grlbwt_round_info *o) {
    const auto &I = e.levels[r].info;
    o->n_in = I.n_in; o->n_phrases = I.D; o->dict_syms = I.S; o->n_metasyms = I.M; o->parse_size = I.parse_size;
    o->sigma = I.sigma; o->max_phrase_len = I.max_phrase_len; o->sort_iters = I.sort_iters;
}
template <class E>
void fill_stats(const E &e, grlbwt_stats *out) {
    const auto &s = e.stats;
    out->n_strings = s.n_strings; out->n_syms = s.n_syms; out->min_sym = s.min_sym; out->max_sym = s.max_sym;
    out->max_sym_freq = s.max_sym_freq; out->sb = s.sb; out->fb = s.fb;
}
template <class E>
void fill_level(const E &e, int l, grlbwt_level_info *o) {
    const auto &I = e.linfo[l];
    o->n = I.n; o->n_runs = I.R; o->runs_next = I.R_next; o->induced_cells = I.E; o->prebwt_runs = I.P;
    o->segments = I.G; o->atoms = I.A; o->chain_steps = I.Esteps; o->merged_cells = I.Emerged;
}
template <class E>
void fill_counters(const E &e, grlbwt_counters *o) {
    memset(o, 0, sizeof(*o));
    const auto &t = e.tm;
    o->t_stats = t.stats; o->t_classify = t.classify; o->t_hash = t.hash; o->t_dict_sort = t.dict_sort;
    o->t_dict_groups = t.dict_groups; o->t_emit = t.emit; o->t_ind_expand = t.ind_expand; o->t_ind_split = t.ind_sort;
    o->t_ind_assemble = t.ind_assemble; o->t_finish = t.finish;
    const uint64_t ib = sizeof(typename std::remove_reference<decltype(e.bwt.len.p[0])>::type);
    o->idx_bytes = ib;
    for (size_t r = 0; r < e.levels.size(); r++) {
        const auto &I = e.levels[r].info;
        o->bytes_classify_hash += I.n_in * (r == 0 ? (uint64_t)e.cell_bytes : 4ull);
        o->bytes_emit += I.parse_size * 4ull;
    }
    for (size_t l = 0; l + 1 < e.linfo.size(); l++) {
        const auto &I = e.linfo[l];
        o->bytes_induce_scatter += I.R_next * (4 + ib) + I.R_next * 4 + I.E * (4 + ib);
        o->bytes_induce_assemble += (I.P + I.E + I.R_next + I.R) * (4 + ib);
    }
}

template <class E>
void text_download(const E &e, int level, uint64_t *out) {
    const auto &b = e.kept_texts[level - 1];
    std::vector<uint32_t> h = b.to_host(b.n);
    for (uint64_t i = 0; i < b.n; i++) out[i] = (uint64_t)(h[i] >> 1);   // (rank<<2|rep<<1|T) -> (rank<<1|rep)
}
template <class E>
void bwt_download(const E &e, int level, uint64_t *sym, uint64_t *len) {
    const auto &b = e.kept_bwts[level];
    auto hs = b.sym.to_host(b.R);
    auto hl = b.len.to_host(b.R);
    for (uint64_t i = 0; i < b.R; i++) { sym[i] = hs[i]; len[i] = hl[i]; }
}

template <class E>
void grammar_download(const E &e, int level, uint64_t *g0, uint64_t *g1, uint8_t *hh, uint64_t *ps, uint64_t *pl) {
    const auto &L = e.levels[level];
    const uint64_t M = L.M, P = L.prebwt.R;
    auto a = L.g0.to_host(M), b = L.g1.to_host(M);
    auto h = L.has_hocc.to_host(M);
    for (uint64_t i = 0; i < M; i++) { if (g0) g0[i] = a[i]; if (g1) g1[i] = b[i]; if (hh) hh[i] = h[i]; }
    auto s = L.prebwt.sym.to_host(P);
    auto l = L.prebwt.len.to_host(P);
    for (uint64_t i = 0; i < P; i++) { if (ps) ps[i] = s[i]; if (pl) pl[i] = l[i]; }
}
#define ENG(ctx, expr) ((ctx)->e32 ? (ctx)->e32->expr : (ctx)->e64->expr)
#define HAS_ENG(ctx) ((ctx) && ((ctx)->e32 || (ctx)->e64))

// GRLBWT_EINVAL before any engine work.  The refusal brings its own message: grlbwt_last_error must not go on showing the text
// of an earlier, unrelated failure.
int refuse(const grlbwt_ctx *ctx, const char *why = "invalid argument, or a call that is out of order for this context") {
    if (ctx) ctx->err = why;
    return GRLBWT_EINVAL;
}
// what a call that needs a text or a finished image is refused with (nullptr: it may go ahead)
const char *need_text(const grlbwt_ctx *ctx) {
    if (!ctx) return "no context";
    if (!HAS_ENG(ctx)) return "no text is loaded in this context";
    if (ENG(ctx, failed)) return "an earlier stage call failed part-way: load the text again";
    return nullptr;
}
const char *need_image(const grlbwt_ctx *ctx) {
    if (const char *why = need_text(ctx)) return why;
    return ENG(ctx, image_bytes) == 0 ? "the build has not finished: there is no image yet" : nullptr;
}
// The stage-wise calls and grlbwt_build (the call-order table of include/grlbwt_hip.h) go through here.  A call the table
// refuses throws before it touches anything, and so does the refusal of a borrowed text that has changed, which comes out
// of the first parsing round: the engine is as it was and the next stage call works.  Any other failure may have left a level
// half made (a round moves the level's text out of the engine while it runs): the engine is marked, and every stage and result
// call returns GRLBWT_EINVAL until a text is loaded again.
template <class Fn>
int stage(grlbwt_ctx *ctx, const char *refused, Fn fn) {
    if (const char *why = need_text(ctx)) return refuse(ctx, why);
    if (refused) return refuse(ctx, refused);
    const int rc = guarded(ctx, fn);
    if (rc != GRLBWT_OK && !ENG(ctx, untouched())) ENG(ctx, mark_failed());
    return rc;
}

static constexpr uint64_t kMergeRowLimit = 1ull << 40;      // grlbwt_merge_create: merged rows, as the build's limit on cells
static constexpr uint64_t kIdx32Limit = 0xFFFFFF00ull;      // texts of this many cells or more take the 64-bit index build
// the index width of a call over n cells, rows or symbols: the 64-bit engine from the limit on, or when the context forces it
static bool idx64_for(const grlbwt_ctx *ctx, uint64_t n) { return n >= kIdx32Limit || (ctx->flags & GRLBWT_FLAG_FORCE_IDX64); }
void load(grlbwt_ctx *ctx, const void *cells, uint64_t n, int w, bool host) {
    ctx->e32.reset();
    ctx->e64.reset();
    bool big = idx64_for(ctx, n);
    bool keep = ctx->flags & GRLBWT_FLAG_KEEP_LEVELS;
    if (big) {
        std::unique_ptr<grl64::Engine> e(new grl64::Engine());
        e->keep_texts = keep;
        if (host) e->upload_text(cells, n, w); else e->load_text(cells, n, w);
        ctx->e64 = std::move(e);          // only a successfully loaded text leaves an engine behind
    } else {
        std::unique_ptr<grl32::Engine> e(new grl32::Engine());
        e->keep_texts = keep;
        if (host) e->upload_text(cells, n, w); else e->load_text(cells, n, w);
        ctx->e32 = std::move(e);
    }
}

// ---- file in / file out: pinned staging buffers, reader/writer threads, copies overlapped with the I/O ---------
// pread/pwrite of [off, off+len) split over `nthr` threads (page-cache copies are memory-bound per thread)
bool par_io(int fd, char *buf, uint64_t off, uint64_t len, bool write, int nthr) {
    auto one = [&](uint64_t a, uint64_t b, bool *ok) {
        while (a < b) {
            ssize_t r = write ? pwrite(fd, buf + (a - off), b - a, (off_t)a) : pread(fd, buf + (a - off), b - a, (off_t)a);
            if (r <= 0) { *ok = false; return; }
            a += (uint64_t)r;
        }
    };
    if (nthr < 1) nthr = 1;
    if (len < ((uint64_t)4 << 20)) nthr = 1;
    if (nthr == 1) { bool ok1 = true; one(off, off + len, &ok1); return ok1; }      // (no thread of its own)
    std::vector<std::thread> th;
    std::vector<char> oks(nthr, 1);
    const uint64_t part = (len + nthr - 1) / nthr;
    for (int t = 0; t < nthr; t++) {
        uint64_t a = off + (uint64_t)t * part, b = a + part < off + len ? a + part : off + len;
        if (a >= b) break;
        th.emplace_back(one, a, b, (bool *)&oks[t]);
    }
    for (auto &x : th) x.join();
    for (char c : oks) if (!c) return false;
    return true;
}
constexpr uint64_t kIoChunk = (uint64_t)64 << 20;
constexpr int kIoBufs = 3;
// reader / writer threads per chunk: page-cache copies run at about 2 GB/s per thread (GRLBWT_IO_THREADS overrides)
int io_threads() {
    const int v = prim::sw().io_threads;
    if (v >= 1 && v <= 64) return v;
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::min<unsigned>(std::max<unsigned>(hc / 2, 4u), 16u);      // (pread from the page cache: 99 GB/s with 8 threads, 118 with 16, 97 with 32 on a 256-core host)
}

// file -> HBM: chunk k+1 is read from the file while chunk k travels over PCIe; for byte cells the histogram of
// collection_stats is taken from every chunk on the device as soon as it has landed (no second pass over the text)
// Reader threads that live for one load: a chunk is cut into 4 MiB pieces which the threads take one by one (pread from the
// page cache: 14 GB/s with one thread, 100-118 GB/s with 8-16 on the GPU box, tools/io_probe.cpp).  (Eight new threads per
// 64 MiB chunk, joined before the next chunk, read the 10 GB input at 43 GB/s.)
struct ReadPool {
    static constexpr uint64_t kPiece = (uint64_t)4 << 20;
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    int fd = -1; char *buf = nullptr; uint64_t off = 0, len = 0;       // the chunk being read
    uint64_t next = 0, done = 0, pieces = 0, generation = 0;
    bool stop = false, ok = true;
    explicit ReadPool(int n) {
        try { for (int i = 0; i < n; i++) th.emplace_back([this] { run(); }); } catch (const std::system_error &) {}      // (as many as there are; none: read() reads in line)
    }
    ~ReadPool() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv_work.notify_all();
        for (auto &t : th) t.join();
    }
    void run() {
        uint64_t seen = 0;
        for (;;) {
            uint64_t p, a, b; int f; char *dst; uint64_t base;
            {
                std::unique_lock<std::mutex> g(mu);
                cv_work.wait(g, [&] { return stop || (generation != seen && next < pieces) ; });
                if (stop) return;
                if (next >= pieces) { seen = generation; continue; }
                p = next++;
                f = fd; dst = buf; base = off;
                a = p * kPiece; b = a + kPiece < len ? a + kPiece : len;
            }
            bool good = true;
            for (uint64_t x = a; x < b && good;) {
                const ssize_t r = pread(f, dst + x, b - x, (off_t)(base + x));
                if (r <= 0) good = false; else x += (uint64_t)r;
            }
            {
                std::lock_guard<std::mutex> g(mu);
                if (!good) ok = false;
                if (++done == pieces) cv_done.notify_all();
            }
        }
    }
    // bytes [off_, off_ + len_) of the file into buf_; returns when they are all there
    bool read(int fd_, char *buf_, uint64_t off_, uint64_t len_) {
        if (th.empty()) return par_io(fd_, buf_, off_, len_, false, 1);
        std::unique_lock<std::mutex> g(mu);
        fd = fd_; buf = buf_; off = off_; len = len_;
        pieces = (len_ + kPiece - 1) / kPiece; next = 0; done = 0; generation++;
        if (pieces == 0) return ok;
        cv_work.notify_all();
        cv_done.wait(g, [&] { return done == pieces; });
        return ok;
    }
};
// GRLBWT_IO_TRACE=1: where the loader and the image writer spend their time (stderr)
inline bool io_trace() { return prim::init_sw().io_trace; }
inline double io_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
template <class E>
void load_file_into(E &e, int fd, uint64_t base, uint64_t bytes, int w) {      // bytes [base, base + bytes) of the file
    const double t_a = io_now();
    e.own0.alloc(bytes + 16);
    const double t_b = io_now();
    double t_read = 0, t_wait = 0;
    char *bufs[kIoBufs] = {nullptr, nullptr, nullptr};
    prim::Fence fences[kIoBufs];
    uint64_t *d_hist = nullptr;
    auto cleanup = [&] {
        for (int k = 0; k < kIoBufs; k++) { prim::fence_destroy(fences[k]); prim::pinned_free(bufs[k]); bufs[k] = nullptr; }
        if (d_hist) prim::dev_free(d_hist);
        d_hist = nullptr;
    };
    try {
        const uint64_t chunk = bytes < kIoChunk ? (bytes + 15) / 16 * 16 : kIoChunk;
        // (the pinned buffers are made as the ring reaches them: pinning 3 x 64 MiB takes 60 ms, and the second and third are not
        // needed before the first chunk is on its way)
        if (w == 1) { d_hist = (uint64_t *)prim::dev_alloc(256 * 8); prim::dev_memset(d_hist, 0, 256 * 8); }
        int k = 0;
        ReadPool pool(bytes > ReadPool::kPiece ? io_threads() : 0);
        for (uint64_t off = 0; off < bytes; off += chunk, k = (k + 1) % kIoBufs) {
            const uint64_t len = bytes - off < chunk ? bytes - off : chunk;
            const double t0 = io_now();
            if (!bufs[k]) bufs[k] = (char *)prim::pinned_alloc(chunk ? chunk : 16);
            prim::fence_wait(fences[k]);                                // the copy that last used this buffer is done
            const double t1 = io_now();
            if (!pool.read(fd, bufs[k], base + off, len)) throw prim::Error(GRLBWT_EINVAL, "cannot read the input file");
            t_wait += t1 - t0; t_read += io_now() - t1;
            prim::h2d_async(e.own0.p + off, bufs[k], len);
            if (d_hist) prim::byte_histogram_accumulate(e.own0.p + off, len, d_hist);
            prim::fence_record(fences[k]);
        }
        uint64_t hist[256];
        const double t_c = io_now();
        if (d_hist) prim::d2h(hist, d_hist, sizeof hist); else prim::sync();
        const double t_d = io_now();
        cleanup();
        if (io_trace()) fprintf(stderr, "[grlbwt] load: device buffer %.3f s, pinned buffers + loop %.3f s (reading %.3f s, waiting for copies %.3f s), drain %.3f s, "
                                        "free %.3f s, %d reader threads\n", t_b - t_a, t_c - t_b, t_read, t_wait, t_d - t_c, io_now() - t_d, io_threads());
        e.load_text(e.own0.p, bytes / (uint64_t)w, w, w == 1 ? hist : nullptr);
    } catch (...) {
        try { prim::sync(); } catch (...) {}
        cleanup();
        throw;
    }
}
void load_file(grlbwt_ctx *ctx, const char *path, int w, uint64_t base = 0, uint64_t range_bytes = ~0ull) {
    ctx->e32.reset();
    ctx->e64.reset();
    if (!(w == 1 || w == 2 || w == 4 || w == 8)) throw prim::Error(GRLBWT_EINVAL, "bad cell width");
    int fd = open(path, O_RDONLY);
    if (fd < 0) throw prim::Error(GRLBWT_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); throw prim::Error(GRLBWT_EINVAL, std::string("cannot stat ") + path); }
    uint64_t bytes = (uint64_t)st.st_size;
    try {
        if (bytes == 0 || bytes % (uint64_t)w) throw prim::Error(GRLBWT_EILLFORMED, "Error: the file is ill formed");
        if (range_bytes != ~0ull) {               // a record shard of the file
            if (base % (uint64_t)w || range_bytes % (uint64_t)w || base > bytes || range_bytes > bytes - base)
                throw prim::Error(GRLBWT_EINVAL, "file range outside the file or not on cell boundaries");
            if (range_bytes == 0) throw prim::Error(GRLBWT_EILLFORMED, "Error: the file is ill formed");
            bytes = range_bytes;
        } else base = 0;
        const uint64_t n = bytes / (uint64_t)w;
        bool big = idx64_for(ctx, n);
        bool keep = ctx->flags & GRLBWT_FLAG_KEEP_LEVELS;
        if (big) {
            std::unique_ptr<grl64::Engine> e(new grl64::Engine());
            e->keep_texts = keep;
            load_file_into(*e, fd, base, bytes, w);
            ctx->e64 = std::move(e);
        } else {
            std::unique_ptr<grl32::Engine> e(new grl32::Engine());
            e->keep_texts = keep;
            load_file_into(*e, fd, base, bytes, w);
            ctx->e32 = std::move(e);
        }
    } catch (...) { close(fd); throw; }
    close(fd);
}
// ---- f3: FASTA/FASTQ files (optionally gzip) ------------------------------------------------------------------------
// gzip iff the file starts with 1F 8B (gzopen's rule, which the reference's converter relies on: fastx_handler.cpp:10)
bool file_magic(const char *path, unsigned char out[2]) {
    int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    out[0] = out[1] = 0;
    ssize_t r = pread(fd, out, 2, 0);
    close(fd);
    return r >= 1;
}
struct RawText { grl64::DBuf<uint8_t> buf; uint64_t n = 0; };
// the (decompressed) bytes of the file in device memory; plain files go through the pinned reader of load_file_into, gzip
// members are inflated on the host (zlib, one stream: the format has no parallel entry points) chunk by chunk into pinned
// buffers that are copied while the next chunk inflates
void read_fastx_raw(const char *path, RawText &R) {
    int fd = open(path, O_RDONLY);
    if (fd < 0) throw prim::Error(GRLBWT_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); throw prim::Error(GRLBWT_EINVAL, std::string("cannot stat ") + path); }
    const uint64_t bytes = (uint64_t)st.st_size;
    unsigned char mg[2] = {0, 0};
    if (bytes >= 2 && pread(fd, mg, 2, 0) != 2) { close(fd); throw prim::Error(GRLBWT_EINVAL, "cannot read the input file"); }
    const bool gz = mg[0] == 0x1F && mg[1] == 0x8B;
    constexpr int NB = 2;
    char *bufs[NB] = {nullptr, nullptr};
    prim::Fence fences[NB];
    std::vector<unsigned char> cin;
    z_stream zs;
    bool z_open = false;
    auto cleanup = [&] {
        for (int k = 0; k < NB; k++) { prim::fence_destroy(fences[k]); prim::pinned_free(bufs[k]); bufs[k] = nullptr; }
        if (z_open) inflateEnd(&zs);
        z_open = false;
        close(fd);
    };
    try {
        const uint64_t chunk = kIoChunk;
        for (int k = 0; k < NB; k++) bufs[k] = (char *)prim::pinned_alloc(chunk);
        if (!gz) {
            R.buf.alloc(bytes + 16);
            int k = 0;
            for (uint64_t off = 0; off < bytes; off += chunk, k = (k + 1) % NB) {
                const uint64_t len = bytes - off < chunk ? bytes - off : chunk;
                prim::fence_wait(fences[k]);
                if (!par_io(fd, bufs[k], off, len, false, io_threads())) throw prim::Error(GRLBWT_EINVAL, "cannot read the input file");
                prim::h2d_async(R.buf.p + off, bufs[k], len);
                prim::fence_record(fences[k]);
            }
            R.n = bytes;
        } else {
            uint64_t cap = bytes * 5 + (1 << 20);
            R.buf.alloc(cap + 16);
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, 15 + 32) != Z_OK) throw prim::Error(GRLBWT_EINTERNAL, "zlib: inflateInit2 failed");
            z_open = true;
            cin.resize((size_t)8 << 20);
            uint64_t in_off = 0, out_n = 0;
            int k = 0;
            prim::fence_wait(fences[k]);
            zs.next_out = (Bytef *)bufs[k]; zs.avail_out = (uInt)chunk;
            auto flush = [&](bool final) {
                const uint64_t len = chunk - zs.avail_out;
                if (len) {
                    if (out_n + len > cap) {                         // grow the device buffer (copy on the engine's stream)
                        const uint64_t ncap = (out_n + len) * 3 / 2 + (1 << 20);
                        grl64::DBuf<uint8_t> nb(ncap + 16);
                        prim::d2d(nb.p, R.buf.p, out_n);
                        R.buf = std::move(nb);
                        cap = ncap;
                    }
                    prim::h2d_async(R.buf.p + out_n, bufs[k], len);
                    prim::fence_record(fences[k]);
                    out_n += len;
                }
                if (!final) {
                    k = (k + 1) % NB;
                    prim::fence_wait(fences[k]);
                    zs.next_out = (Bytef *)bufs[k]; zs.avail_out = (uInt)chunk;
                }
            };
            bool done = false;
            while (!done) {
                if (zs.avail_in == 0) {
                    if (in_off >= bytes) break;
                    const uint64_t len = bytes - in_off < cin.size() ? bytes - in_off : cin.size();
                    if (!par_io(fd, (char *)cin.data(), in_off, len, false, 1)) throw prim::Error(GRLBWT_EINVAL, "cannot read the input file");
                    in_off += len;
                    zs.next_in = cin.data(); zs.avail_in = (uInt)len;
                }
                const int r = inflate(&zs, Z_NO_FLUSH);
                if (r == Z_STREAM_END) {
                    // another member follows only if the bytes behind this one start with the gzip magic; anything else
                    // (zero padding of blocked / tape files, stray bytes) is ignored, as gzread does
                    if (zs.avail_in < 2 && in_off < bytes) {          // the two bytes may straddle a read: pull more behind the leftover
                        const size_t keep = zs.avail_in;
                        if (keep) memmove(cin.data(), zs.next_in, keep);
                        const uint64_t len = bytes - in_off < cin.size() - keep ? bytes - in_off : cin.size() - keep;
                        if (!par_io(fd, (char *)cin.data() + keep, in_off, len, false, 1)) throw prim::Error(GRLBWT_EINVAL, "cannot read the input file");
                        in_off += len;
                        zs.next_in = cin.data(); zs.avail_in = (uInt)(keep + len);
                    }
                    if (zs.avail_in >= 2 && zs.next_in[0] == 0x1F && zs.next_in[1] == 0x8B) {
                        if (inflateReset(&zs) != Z_OK) throw prim::Error(GRLBWT_EINTERNAL, "zlib: inflateReset failed");
                    } else done = true;
                } else if (r != Z_OK && r != Z_BUF_ERROR) {
                    throw prim::Error(GRLBWT_EINVAL, std::string("the gzip stream is damaged (zlib: ") + (zs.msg ? zs.msg : "error") + ")");
                } else if (r == Z_BUF_ERROR && zs.avail_in == 0 && in_off >= bytes) done = true;       // truncated file: take what there is (gzread does)
                if (zs.avail_out == 0) flush(false);
            }
            flush(true);
            R.n = out_n;
        }
        prim::sync();
        cleanup();
    } catch (...) {
        try { prim::sync(); } catch (...) {}
        cleanup();
        throw;
    }
}
// an .rl_bwt file in device memory (grlbwt_merge_files): the plain-file branch of the reader above -- an image starts with its
// symbol width, 1 to 8, never with the gzip magic
void read_image_file(const char *path, RawText &R) {
    unsigned char mg[2] = {0, 0};
    if (!file_magic(path, mg)) throw prim::Error(GRLBWT_EINVAL, std::string("cannot open ") + path);
    if (mg[0] == 0x1F && mg[1] == 0x8B) throw prim::Error(GRLBWT_EINVAL, std::string(path) + " is a gzip file, not an .rl_bwt image");
    read_fastx_raw(path, R);
}
void load_fastx(grlbwt_ctx *ctx, const char *path, uint32_t fx_flags, uint64_t *n_strings) {
    ctx->e32.reset();
    ctx->e64.reset();
    RawText raw;
    read_fastx_raw(path, raw);
    const bool rc = (fx_flags & GRLBWT_FASTX_REVCOMP) != 0;
    const uint64_t cap = (rc ? 2 : 1) * raw.n + 16;
    grl64::DBuf<uint8_t> text(cap + 16);
    grl64::Engine::FastxInfo info = grl64::Engine::fastx_to_text(raw.buf.p, raw.n, rc, text.p, cap);
    raw.buf.release();
    if (n_strings) *n_strings = info.n_strings;
    if (info.n_out == 0) throw prim::Error(GRLBWT_EILLFORMED, "Error: the file is ill formed");      // no record at all
    const uint64_t n = info.n_out;
    bool big = idx64_for(ctx, n);
    bool keep = ctx->flags & GRLBWT_FLAG_KEEP_LEVELS;
    if (big) {
        std::unique_ptr<grl64::Engine> e(new grl64::Engine());
        e->keep_texts = keep;
        e->own0 = std::move(text);
        e->load_text(e->own0.p, n, 1);
        ctx->e64 = std::move(e);
    } else {
        std::unique_ptr<grl32::Engine> e(new grl32::Engine());
        e->keep_texts = keep;
        e->own0.alloc(n + 16);                                        // (the two engines have their own buffer types)
        prim::d2d(e->own0.p, text.p, n);
        text.release();
        e->load_text(e->own0.p, n, 1);
        ctx->e32 = std::move(e);
    }
}
// HBM image -> file.  A buffered write to ONE file runs at the rate of one thread copying into the page cache, whatever the
// number of threads (the inode's lock; tools/io_probe.cpp on the GPU box, 8 GiB to /tmp: 1 thread 10.9 GB/s, 4-16 threads with
// pwrite on disjoint ranges 9.3-9.7, 64 threads 3.8, preallocated with posix_fallocate 11.1, O_DIRECT 7.1 -- and 64 GB/s into
// EIGHT files; a shared mapping filled by 16 threads was 4x slower: page faults).  So: the blocks are preallocated, ONE writer
// thread lives for the whole image and writes the chunks in order as their copies land in a ring of pinned buffers; the device
// copies (50+ GB/s) stay ahead of it.  (Before: a writer thread per 64 MiB chunk that started eight more: 0.97-1.17 s for the
// 8.3 GB image of the 10 GB build.)
// (part = true: the nb bytes go to offset file_off of `path` itself, created if needed and never truncated -- one of N ranks
// writing one file, grlbwt_result_write_part; publishing the complete file is the caller's business)
void write_image(const uint8_t *dev_image, uint64_t nb, const char *path, bool part = false, uint64_t file_off = 0, uint64_t image_total = 0) {
    // The image goes to <path>.tmp~<pid> and is renamed over the target once it is complete and closed (the reference renames
    // bwt_lev_0 to the output name, grl_bwt.hpp:77): an existing output stays intact until then, and a run that is killed or fails
    // leaves at most the temporary behind -- removed on every error path here.  What replacing an existing output costs is the
    // release of its cached pages inside rename() (~0.6 s for 8.3 GB).
    const double t_a = io_now();
    const std::string tmp = part ? std::string(path) : std::string(path) + ".tmp~" + std::to_string((long)getpid());
    int fd = open(tmp.c_str(), part ? (O_WRONLY | O_CREAT) : (O_WRONLY | O_CREAT | O_TRUNC), 0644);
    if (fd < 0) throw prim::Error(GRLBWT_EINVAL, std::string("cannot open ") + tmp);
    constexpr int NBUF = 4;
    char *bufs[NBUF] = {nullptr, nullptr, nullptr, nullptr};
    prim::Fence fences[NBUF];
    struct Job { uint64_t off, len; };
    Job jobs[NBUF];
    std::mutex mu;
    std::condition_variable cv;
    int filled = 0, written = 0;              // chunks handed to the writer / chunks it has finished (ring positions = count % NBUF)
    bool stop = false;
    std::atomic<bool> ok(true);
    std::thread writer;                       // outside the try block: a failing copy must not unwind past a joinable thread
    double t_wait_copy = 0, t_pwrite = 0;
    auto finish_writer = [&] {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv.notify_all();
        if (writer.joinable()) writer.join();
    };
    try {
        const uint64_t chunk = nb < kIoChunk ? nb : kIoChunk;
        if (!part && nb && posix_fallocate(fd, 0, (off_t)nb) != 0 && ftruncate(fd, (off_t)nb) != 0) ok = false;
        const double t_b = io_now();
        auto body = [&] {
            prim::thread_attach();
            for (;;) {
                int k;
                Job j;
                {
                    std::unique_lock<std::mutex> g(mu);
                    cv.wait(g, [&] { return stop || written < filled; });
                    if (written >= filled) return;                   // (stop, nothing left)
                    k = written % NBUF;
                    j = jobs[k];
                }
                const double t0 = io_now();
                try { prim::fence_wait(fences[k]); } catch (...) { ok = false; }
                const double t1 = io_now();
                if (ok && !par_io(fd, bufs[k], file_off + j.off, j.len, true, 1)) ok = false;
                t_wait_copy += t1 - t0; t_pwrite += io_now() - t1;
                { std::lock_guard<std::mutex> g(mu); written++; }
                cv.notify_all();
            }
        };
        try { writer = std::thread(body); } catch (const std::system_error &) { /* no thread to be had: the chunks are written below */ }
        for (uint64_t off = 0; off < nb && ok; off += chunk) {
            const uint64_t len = nb - off < chunk ? nb - off : chunk;
            int k;
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return filled - written < NBUF; });         // a free buffer
                k = filled % NBUF;
            }
            if (!bufs[k]) bufs[k] = (char *)prim::pinned_alloc(chunk ? chunk : 16);      // (made as the ring reaches them: the writer is busy by then)
            prim::d2h_async(bufs[k], dev_image + off, len);
            prim::fence_record(fences[k]);
            if (writer.joinable()) {
                { std::lock_guard<std::mutex> g(mu); jobs[k] = Job{off, len}; filled++; }
                cv.notify_all();
            } else {                                                          // (no writer thread: in line)
                prim::fence_wait(fences[k]);
                if (!par_io(fd, bufs[k], file_off + off, len, true, 1)) ok = false;
            }
        }
        {   // everything handed over: wait for the writer to drain
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return written >= filled; });
        }
        finish_writer();
        if (io_trace()) fprintf(stderr, "[grlbwt] write: open + buffers + preallocation %.3f s, chunks %.3f s (writer: waiting for copies %.3f s, writing %.3f s)\n",
                                t_b - t_a, io_now() - t_b, t_wait_copy, t_pwrite);
    } catch (...) {
        finish_writer();
        try { prim::sync(); } catch (...) {}
        for (int k = 0; k < NBUF; k++) { prim::fence_destroy(fences[k]); prim::pinned_free(bufs[k]); }
        close(fd);
        if (!part) unlink(tmp.c_str());
        throw;
    }
    for (int k = 0; k < NBUF; k++) { prim::fence_destroy(fences[k]); prim::pinned_free(bufs[k]); }
    // (a part: the rank whose part ends the image gives the file its size -- a longer file that was there before, a caller that
    // reuses a path, keeps no stale tail)
    if (ok && part && image_total && file_off + nb == image_total && ftruncate(fd, (off_t)image_total) != 0) ok = false;
    if (close(fd) != 0) ok = false;
    if (ok && !part && rename(tmp.c_str(), path) != 0) ok = false;
    if (!ok) { if (!part) unlink(tmp.c_str()); throw prim::Error(GRLBWT_EINVAL, std::string("short write to ") + path); }
}

// ---- primitive self-test (device vs host loops) -----------------------------
uint64_t sm64(uint64_t &s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
struct OddPred {
    const uint32_t *v;
    GRL_DEV bool operator()(uint64_t i) const { return (v[i] % 3u) == 1u; }
};
struct U32In {
    const uint32_t *v;
    GRL_DEV uint64_t operator()(uint64_t i) const { return (uint64_t)(v[i] & 1023u); }
};
struct U32Raw {
    const uint32_t *v;
    GRL_DEV uint32_t operator()(uint64_t i) const { return v[i]; }
};

template <class A, class B>
struct PairOfIn {
    const uint32_t *v;
    GRL_DEV prim::Pair<A, B> operator()(uint64_t i) const { return prim::Pair<A, B>((A)(v[i] & 1u), (B)(v[i] & 4095u)); }
};
template <class A, class B>
int test_pair_scan(uint64_t n, const std::vector<uint32_t> &h, const uint32_t *d) {
    typedef prim::Pair<A, B> P;
    grl32::DBuf<P> o(n + 1);
    P tot = prim::exclusive_scan<P>(n, PairOfIn<A, B>{d}, o.p, true, "selftest.pairscan");
    std::vector<P> ho = o.to_host(n + 1);
    A a = 0; B b = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (ho[i].a != a || ho[i].b != b) return 1;
        a += (A)(h[i] & 1u); b += (B)(h[i] & 4095u);
    }
    if (ho[n].a != a || ho[n].b != b || tot.a != a || tot.b != b) return 2;
    return 0;
}

int test_sort_keys(uint64_t n, uint64_t seed, int bits) {       // keys-only sort on the low `bits` bits: stability through the high bits
    std::vector<uint64_t> hk(n);
    uint64_t s = seed;
    uint64_t mask = (1ull << bits) - 1;
    for (uint64_t i = 0; i < n; i++) hk[i] = (sm64(s) & mask) | (i << bits);       // original index rides above the sorted bits
    grl32::DBuf<uint64_t> ka(n), kb(n);
    prim::h2d(ka.p, hk.data(), n * 8);
    int res = prim::sort_keys<uint64_t>(ka.p, kb.p, n, 0, bits, "selftest.sort_keys");
    std::vector<uint64_t> ok = (res ? kb : ka).to_host(n);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t idx = ok[i] >> bits;
        if (idx >= n || hk[idx] != ok[i]) return 1;
        if (i > 0 && (ok[i - 1] & mask) > (ok[i] & mask)) return 2;
        if (i > 0 && (ok[i - 1] & mask) == (ok[i] & mask) && (ok[i - 1] >> bits) >= idx) return 3;
    }
    return 0;
}

template <class K, class V>
int test_sort(uint64_t n, uint64_t seed, int bits) {
    std::vector<K> hk(n);
    std::vector<V> hv(n);
    uint64_t s = seed;
    K mask = bits >= (int)(8 * sizeof(K)) ? ~K(0) : (K)((K(1) << bits) - 1);
    for (uint64_t i = 0; i < n; i++) { hk[i] = (K)sm64(s) & mask; hv[i] = (V)i; }
    grl32::DBuf<K> ka(n), kb(n);
    grl32::DBuf<V> va(n), vb(n);
    prim::h2d(ka.p, hk.data(), n * sizeof(K));
    prim::h2d(va.p, hv.data(), n * sizeof(V));
    int res = prim::sort_pairs<K, V>(ka.p, va.p, kb.p, vb.p, n, 0, bits, "selftest.sort");
    std::vector<K> ok = (res ? kb : ka).to_host(n);
    std::vector<V> ov = (res ? vb : va).to_host(n);
    for (uint64_t i = 0; i < n; i++) {
        if (ok[i] != hk[(uint64_t)ov[i]]) return 1;                          // pair integrity
        if (i > 0 && ok[i - 1] > ok[i]) return 2;                            // order
        if (i > 0 && ok[i - 1] == ok[i] && ov[i - 1] >= ov[i]) return 3;     // stability
    }
    return 0;
}

struct SelfValid {
    GRL_DEV bool operator()(uint64_t hi) const { return (hi >> 61) != 0; }
};
// RecSort (forward, backward) + rec_dedupe against host containers
int test_part(uint64_t n, uint64_t seed, int pbits) {
    while (pbits < 20 && (n >> pbits) > 3000) pbits++;          // partitions that fit the LDS table (as the engine sizes them)
    std::vector<uint64_t> hk(n), hh(n);
    uint64_t s = seed;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t r = sm64(s);
        const uint64_t id = r % (n / 3 + 1);                                          // ~3 records per distinct value
        if (r % 11 == 0) { hk[i] = i; hh[i] = 0; }                                    // invalid record
        else { hh[i] = (id % 5) | (3ull << 61); hk[i] = (id * 0x9E3779B97F4A7C15ull) ^ (hh[i] * 0xD6E8FEB86659FD93ull); }
    }
    grl32::DBuf<uint64_t> ka(n), ha(n), kb(n), hb(n), dkey(n), dhi(n);
    grl32::DBuf<uint32_t> wa(n), wb(n), wc(n), lid(n), dcnt(n);
    prim::h2d(ka.p, hk.data(), n * 8);
    prim::h2d(ha.p, hh.data(), n * 8);
    prim::RecSort ps;
    const int res = ps.forward(ka.p, ha.p, kb.p, hb.p, n, pbits, "selftest.part");
    std::vector<uint64_t> sk = (res ? kb : ka).to_host(n), sh = (res ? hb : ha).to_host(n);
    {   // a permutation of the input pairs, grouped by partition, stable inside a partition
        std::map<std::pair<uint64_t, uint64_t>, int64_t> bal;
        for (uint64_t i = 0; i < n; i++) bal[{hk[i], hh[i]}]++;
        for (uint64_t j = 0; j < n; j++) {
            if (j && prim::RecSort::part_of(sk[j - 1], pbits) > prim::RecSort::part_of(sk[j], pbits)) return 1;
            if (--bal[{sk[j], sh[j]}] < 0) return 2;                                  // keys and values moved together
        }
    }
    // backward: an element per sorted record returns to the record's original place
    std::vector<uint32_t> hw(n);
    for (uint64_t j = 0; j < n; j++) hw[j] = (uint32_t)(sk[j] * 31 + sh[j]);
    prim::h2d(wa.p, hw.data(), n * 4);
    ps.backward(wa.p, wb.p, wc.p, "selftest.part_back");
    std::vector<uint32_t> ho = wc.to_host(n);
    for (uint64_t i = 0; i < n; i++) if (ho[i] != (uint32_t)(hk[i] * 31 + hh[i])) return 3;
    // per-partition de-duplication
    const uint64_t nparts = (uint64_t)1 << pbits;
    grl32::DBuf<uint64_t> pstart(nparts + 1);
    grl32::DBuf<uint32_t> pcount(nparts), ovf(1);
    ovf.zero();
    prim::for_each(nparts + 1, prim::RecBoundsFn{res ? kb.p : ka.p, n, pbits, nparts, pstart.p}, "selftest.bounds");
    prim::rec_dedupe(nparts, pstart.p, res ? kb.p : ka.p, res ? hb.p : ha.p, SelfValid{}, lid.p, pcount.p, dkey.p, dhi.p, dcnt.p, ovf.p, "selftest.dedupe");
    if (ovf.get(0)) return 4;
    std::vector<uint64_t> hp = pstart.to_host(nparts + 1), hdk = dkey.to_host(n), hdh = dhi.to_host(n);
    std::vector<uint32_t> hl = lid.to_host(n), hc = pcount.to_host(nparts), hdc = dcnt.to_host(n);
    if (hp[0] != 0 || hp[nparts] != n) return 10;
    for (uint64_t p = 0; p < nparts; p++) {
        std::map<std::pair<uint64_t, uint64_t>, uint32_t> seen;
        for (uint64_t i = hp[p]; i < hp[p + 1]; i++) {
            if (prim::RecSort::part_of(sk[i], pbits) != p) return 11;
            if ((sh[i] >> 61) == 0) { if (hl[i] != prim::kNoId) return 5; continue; }
            seen[{sk[i], sh[i]}]++;
            if (hl[i] >= hc[p]) return 6;
            if (hdk[hp[p] + hl[i]] != sk[i] || hdh[hp[p] + hl[i]] != sh[i]) return 7;    // the local id names the record's value
        }
        if (seen.size() != hc[p]) return 8;
        for (uint32_t j = 0; j < hc[p]; j++) if (seen[{hdk[hp[p] + j], hdh[hp[p] + j]}] != hdc[hp[p] + j]) return 9;
    }
    return 0;
}

// ---- self-test, second part: stream merge, LDS segment sort, record packing, set-bit walk ------------------------------
// Every section has a host reference of its own written from plain arrays (none goes through the functors handed to the device,
// prim::sm_walk or the serial stand-in), poisons what the device may write and checks that nothing else changed.  A mismatch
// prints one line with everything needed to find it; the return code names the section (-2xx, -3xx, -4xx, -5xx).
GRL_HD uint64_t self_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t self_size(uint64_t n) { return std::min<uint64_t>(n, ((uint64_t)1 << 21) + n % 4099); }      // sizes taken from n stay bounded
template <class T>
void self_upload(grl32::DBuf<T> &d, const std::vector<T> &h) {
    d.alloc(h.size());
    prim::h2d(d.p, h.data(), h.size() * sizeof(T));
}
struct alignas(16) SelfRank { uint64_t w, b; };      // a word of a bit-vector and the set bits in front of it
std::vector<SelfRank> self_rank_cells(const std::vector<uint64_t> &words) {
    std::vector<SelfRank> c(words.size());
    uint64_t b = 0;
    for (size_t i = 0; i < words.size(); i++) { c[i].w = words[i]; c[i].b = b; b += (uint64_t)__builtin_popcountll(words[i]); }
    return c;
}

// ---- 1: stream merge
// The segment stream in the shape of the engine's AsmSeg: "pre" runs and "cells" (two record arrays), a bit-vector over the
// segment axis that says which is which, and T given by its maximal runs (start bits with ranks, symbols, positions).
// Lengths are >= 1: a TAKE of no symbols would underflow the kernel's `kb - 1 - ka`, and the engine makes none.
static constexpr uint32_t kSelfTake = 0x3FFFFFFFu;
static const uint32_t kSelfSyms[3] = {0u, 1u, 0x3FFFFFFEu};
template <class IDX>
struct SelfSeg {
    const SelfRank *kinds; const uint32_t *pre_sym; const IDX *pre_len; const uint32_t *cell_sym; const IDX *cell_len; uint32_t take_code;
    const SelfRank *tstarts; const uint32_t *esym_; const IDX *epos_;
    struct Ref { uint64_t idx; bool pre; };
    GRL_DEV static uint64_t rank(const SelfRank *rc, uint64_t x) {
        const SelfRank c = rc[x >> 6];
        return c.b + (uint64_t)__builtin_popcountll(c.w & ((1ull << (x & 63)) - 1ull));
    }
    GRL_DEV Ref locate(uint64_t g) const {
        const uint64_t ord = rank(kinds, g);
        const bool pre = (kinds[g >> 6].w >> (g & 63)) & 1ull;
        return Ref{pre ? ord : g - ord, pre};
    }
    GRL_DEV void fetch(const Ref &r, uint32_t &sym, IDX &len, bool &take) const {
        if (r.pre) { sym = pre_sym[r.idx]; len = pre_len[r.idx]; }
        else { sym = cell_sym[r.idx]; len = cell_len[r.idx]; }
        take = sym == take_code;
    }
    GRL_DEV uint64_t pre_before(uint64_t g) const { return rank(kinds, g); }
    GRL_DEV Ref plain(uint64_t t) const { return Ref{t, false}; }
    GRL_DEV uint64_t erank(uint64_t x) const { return rank(tstarts, x); }
    GRL_DEV void eword(uint64_t w, uint64_t &bits, uint64_t &before) const { const SelfRank c = tstarts[w]; bits = c.w; before = c.b; }
    GRL_DEV uint32_t esym(uint64_t k) const { return esym_[k]; }
    GRL_DEV uint64_t epos(uint64_t k) const { return (uint64_t)epos_[k]; }
};
// A scenario: the segments in output order and T's maximal runs.  T grows as the TAKE segments consume it, so the TAKE lengths
// always tile it; a new run never repeats the symbol of the one in front of it, so the runs are maximal.
struct SmScn {
    const char *name = "";
    std::vector<uint8_t> pre;              // segment g is a pre run (else a cell)
    std::vector<uint32_t> sym;             // kSelfTake: a TAKE
    std::vector<uint64_t> len;
    std::vector<uint32_t> tsym;
    std::vector<uint64_t> tlen;
    uint32_t tcur = 0xFFFFFFFFu;           // symbol of T's run in progress
    uint64_t trem = 0;                     // symbols it still has to hand out
    uint32_t tmaxrun = 4;
    uint64_t rng = 1;
    int idx_only = 0;                      // 4 / 8: the scenario is made for one index width
    // what the scenario is there for: each must be seen at least once (per tile size) or the scenario has lost its point
    bool need_plain = false, need_mixed = false, need_unstaged = false, need_queued = false, need_staged_queued = false, need_wide = false,
         need_exact = false, need_zero = false, need_ends = false, need_one_run = false, need_inner = false;
    int ends_hit = 0;
    uint64_t r() { return sm64(rng); }
    void lit(uint32_t s, uint64_t l, bool p) { pre.push_back(p ? 1 : 0); sym.push_back(s); len.push_back(l); }
    void t_run(uint32_t s, uint64_t l) { tsym.push_back(s); tlen.push_back(0); tcur = s; trem = l; }      // (s differs from tcur; the run in progress ends where it is)
    uint32_t other(uint32_t s) { uint32_t o; do o = kSelfSyms[r() % 3]; while (o == s); return o; }
    void take(uint64_t l, bool p) {
        pre.push_back(p ? 1 : 0); sym.push_back(kSelfTake); len.push_back(l);
        while (l) {
            if (!trem) t_run(other(tcur), 1 + r() % tmaxrun);
            const uint64_t c = std::min(l, trem);
            tlen.back() += c; trem -= c; l -= c;
        }
    }
    // the literal at `giant` gets the length that makes the segments [a, b) describe exactly `total` symbols
    void fit(uint64_t a, uint64_t b, uint64_t giant, uint64_t total) {
        uint64_t s = 0;
        for (uint64_t g = a; g < b && g < len.size(); g++) if (g != giant) s += len[g];
        len[giant] = total - s;
    }
};
struct SmRef {
    std::vector<uint32_t> rsym;
    std::vector<uint64_t> rstart;
    std::vector<uint64_t> run0;            // [G + 1] runs in front of segment g
    std::vector<uint32_t> inner;           // [G] runs of T a TAKE touches behind the first
    uint64_t take_total = 0, len_total = 0, atoms = 0;
};
// the run-level serial walk: literal runs and the pieces of T's runs the TAKE segments cut out, equal neighbours merged
void sm_reference(const SmScn &sc, SmRef &R) {
    const uint64_t G = sc.sym.size();
    R.run0.assign(G + 1, 0);
    R.inner.assign(G, 0);
    uint64_t x = 0, L = 0, tstart = 0;
    size_t tk = 0;
    uint32_t prev = 0xFFFFFFFFu;
    for (uint64_t g = 0; g < G; g++) {
        R.run0[g] = R.rsym.size();
        if (sc.sym[g] != kSelfTake) {
            R.atoms++;
            if (sc.sym[g] != prev) { R.rsym.push_back(sc.sym[g]); R.rstart.push_back(L); }
            prev = sc.sym[g];
        } else {
            const uint64_t end = x + sc.len[g];
            uint32_t pieces = 0;
            for (uint64_t at = x; at < end;) {
                while (tstart + sc.tlen[tk] <= at) { tstart += sc.tlen[tk]; tk++; }      // the run of T that holds `at`
                const uint32_t s = sc.tsym[tk];
                R.atoms++; pieces++;
                if (s != prev) { R.rsym.push_back(s); R.rstart.push_back(L + (at - x)); }
                prev = s;
                at = std::min(end, tstart + sc.tlen[tk]);
            }
            R.inner[g] = pieces - 1;
            x = end;
        }
        L += sc.len[g];
    }
    R.run0[G] = R.rsym.size();
    R.take_total = x; R.len_total = L;
}
// the same from the symbol string itself (small totals): expand T, expand the segments, run-length encode
bool sm_reference_agrees_with_expansion(const SmScn &sc, const SmRef &R) {
    std::vector<uint32_t> T, S;
    T.reserve(R.take_total); S.reserve(R.len_total);
    for (size_t k = 0; k < sc.tsym.size(); k++) T.insert(T.end(), sc.tlen[k], sc.tsym[k]);
    if (T.size() != R.take_total) return false;
    uint64_t x = 0;
    for (size_t g = 0; g < sc.sym.size(); g++) {
        if (sc.sym[g] != kSelfTake) S.insert(S.end(), sc.len[g], sc.sym[g]);
        else { S.insert(S.end(), T.begin() + x, T.begin() + x + sc.len[g]); x += sc.len[g]; }
    }
    if (S.size() != R.len_total || x != R.take_total) return false;
    size_t k = 0;
    for (uint64_t i = 0; i < S.size(); i++) {
        if (i && S[i] == S[i - 1]) continue;
        if (k >= R.rsym.size() || R.rsym[k] != S[i] || R.rstart[k] != i) return false;
        k++;
    }
    return k == R.rsym.size();
}
struct SmTileStats { uint64_t tiles = 0, plain = 0, mixed = 0, unstaged = 0, queued = 0, staged_queued = 0, wide = 0, exact_fe = 0, exact_ff = 0, zero = 0; };
SmTileStats sm_tile_stats(const SmScn &sc, const SmRef &R, int spt, int idx_bytes) {
    const uint64_t G = sc.sym.size(), tile = 256ull * (uint64_t)spt;
    SmTileStats st;
    for (uint64_t a = 0; a < G; a += tile) {
        const uint64_t b = std::min(G, a + tile), heads = R.run0[b] - R.run0[a];
        uint64_t npre = 0, total = 0, q = 0;
        for (uint64_t g = a; g < b; g++) { npre += sc.pre[g]; total += sc.len[g]; if (R.inner[g] > 8) q++; }
        st.tiles++;
        if (npre) st.mixed++; else st.plain++;
        if (heads > tile) st.unstaged++;
        else if (a > 0) st.staged_queued += q;
        st.queued += q;
        if (idx_bytes == 8 && total >= 0xFFFFFFFFull) st.wide++;
        if (total == 0xFFFFFFFEull) st.exact_fe++;
        if (total == 0xFFFFFFFFull) st.exact_ff++;
        if (heads == 0) st.zero++;
    }
    return st;
}
// 0, or what the scenario declared and did not get
const char *sm_scenario_lost(const SmScn &sc, const SmRef &R, int spt, int idx_bytes) {
    const SmTileStats st = sm_tile_stats(sc, R, spt, idx_bytes);
    if (sc.need_plain && st.plain < 3) return "plain tiles";
    if (sc.need_mixed && !st.mixed) return "mixed tiles";
    if (sc.need_unstaged && !st.unstaged) return "tiles with more heads than segments";
    if (sc.need_queued && !st.queued) return "queued segments";
    if (sc.need_staged_queued && !st.staged_queued) return "queued segments in a staged tile behind the first";
    if (sc.need_wide && !st.wide) return "tiles in the 64-bit form";
    if (sc.need_exact && (!st.exact_fe || !st.exact_ff)) return "tiles of exactly 2^32 - 2 and 2^32 - 1 symbols";
    if (sc.need_zero && st.zero + 1 != st.tiles) return "tiles without a head";
    if (sc.need_ends && sc.ends_hit != 5) return "TAKE ends at T bits 63, 64, 65, 127, 128";
    if (sc.need_one_run && R.rsym.size() != 1) return "a single run";
    if (sc.need_inner) {
        bool seen[10] = {false};
        for (uint32_t v : R.inner) if (v < 10) seen[v] = true;
        if (!seen[0] || !seen[1] || !seen[8] || !seen[9]) return "TAKEs with 0, 1, 8 and 9 inner runs";
    }
    return nullptr;
}

SmScn sm_scn_mix(uint64_t G, uint64_t seed) {
    SmScn sc;
    sc.name = "mix"; sc.rng = seed;
    static const uint64_t ends[5] = {63, 64, 65, 127, 128};      // a TAKE's end in the word of its start, at its last bit, in the next word
    uint64_t x = 0, left = 3000 + sc.r() % 2000;
    bool mixed = true, first = true;
    for (uint64_t g = 0; g < G; g++) {
        if (!left) { mixed = !mixed; first = true; left = mixed ? 3000 + sc.r() % 2000 : 4 * 2048 + sc.r() % 3000; }
        const bool p = mixed && (first || sc.r() % 3 == 0);
        if (sc.r() % 4 == 0) {
            uint64_t l = 1 + sc.r() % 5;
            if (sc.ends_hit < 5 && x < ends[sc.ends_hit] && ends[sc.ends_hit] - x <= 5) l = ends[sc.ends_hit] - x;
            sc.take(l, p);
            x += l;
            if (sc.ends_hit < 5 && x == ends[sc.ends_hit]) sc.ends_hit++;
        } else sc.lit(kSelfSyms[sc.r() % 3], 1 + sc.r() % 5, p);
        first = false; left--;
    }
    sc.need_mixed = true;
    sc.need_plain = G >= 16384;          // (a mixed stretch is at most 5000 segments, the plain one behind it at least four large tiles)
    sc.need_ends = G >= 4096;
    return sc;
}
SmScn sm_scn_one_run(uint64_t seed) {
    SmScn sc;
    sc.name = "one run"; sc.rng = seed;
    for (uint64_t g = 0; g < 3 * 2048 + 5; g++) sc.lit(kSelfSyms[1], 1 + sc.r() % 3, sc.r() % 3 == 0);
    sc.need_zero = sc.need_one_run = sc.need_mixed = true;
    return sc;
}
SmScn sm_scn_seam(uint64_t seed) {
    SmScn sc;
    sc.name = "tile seam"; sc.rng = seed;
    const uint64_t G = 5 * 1024 + 17;
    uint32_t forced = 0xFFFFFFFFu;
    for (uint64_t g = 0; g < G; g++) {
        const bool p = sc.r() % 3 == 0;
        if ((g + 1) % 1024 == 0) {           // the last segment of a small tile, of a large one too where (g + 1) / 1024 is even
            const uint64_t k = (g + 1) / 1024;
            const uint32_t s = sc.other(sc.tcur);
            sc.t_run(s, 5);                  // the TAKE takes two of its five symbols: it ends inside the run
            sc.take(2, p);
            forced = (k == 3 || k == 4) ? sc.other(s) : s;
        } else if (forced != 0xFFFFFFFFu) { sc.lit(forced, 1 + sc.r() % 3, p); forced = 0xFFFFFFFFu; }
        else if (sc.r() % 4 == 0) sc.take(1 + sc.r() % 5, p);
        else sc.lit(kSelfSyms[sc.r() % 3], 1 + sc.r() % 3, p);
    }
    sc.need_mixed = true;
    return sc;
}
SmScn sm_scn_wide(uint64_t seed) {
    SmScn sc;
    sc.name = "wide"; sc.rng = seed; sc.tmaxrun = 1;       // runs of one symbol: a TAKE of l symbols has l - 1 inner runs
    const uint64_t G = 4 * 2048 + 100;
    static const uint64_t lens[4] = {1, 2, 9, 10};
    uint32_t forced = 0xFFFFFFFFu, last = kSelfSyms[0];
    for (uint64_t g = 0; g < G; g++) {
        const bool p = sc.r() % 3 == 0;
        if (g == 0 || g == 4095 || g == 4096 + 100 || g == 4096 + 600) { sc.take(5001, p); forced = sc.tcur; }
        else if (forced != 0xFFFFFFFFu) { sc.lit(forced, 1 + sc.r() % 3, p); last = forced; forced = 0xFFFFFFFFu; }
        else if (sc.r() % 16 == 0) sc.take(lens[sc.r() % 4], p);
        else { if (sc.r() % 2) last = kSelfSyms[sc.r() % 3]; sc.lit(last, 1 + sc.r() % 3, p); }
    }
    sc.need_unstaged = sc.need_queued = sc.need_staged_queued = sc.need_inner = sc.need_mixed = true;
    return sc;
}
SmScn sm_scn_random(const char *name, uint64_t G, uint64_t seed) {
    SmScn sc;
    sc.name = name; sc.rng = seed;
    for (uint64_t g = 0; g < G; g++) {
        const bool p = sc.r() % 3 == 0;
        if (sc.r() % 4 == 0) sc.take(1 + sc.r() % 5, p);
        else sc.lit(kSelfSyms[sc.r() % 3], 1 + sc.r() % 3, p);
    }
    return sc;
}
SmScn sm_scn_wide64(uint64_t seed) {
    // Counted in small tiles of 1024 segments (small tile b lies in large tile b / 2).  A giant literal makes large tile 1 and small
    // tile 6 describe exactly 2^32 - 2 symbols (the last tiles of the 32-bit form), large tile 5 and small tile 14 exactly 2^32 - 1
    // (the first of the 64-bit form), and small tiles 18 and 19 hold literals of 2^31 .. 2^33.  The tiles between them stay small.
    // A giant takes the place of the first literal at or behind its offset, so the TAKE segments and the T axis stay as drawn.
    SmScn sc = sm_scn_random("64-bit tiles", 21 * 1024 + 300, seed);
    sc.idx_only = 8;
    auto lit_at = [&](uint64_t g) { while (sc.sym[g] == kSelfTake) g++; return g; };
    const uint64_t g1 = lit_at(2 * 1024 + 5), g2 = lit_at(6 * 1024 + 5), g3 = lit_at(10 * 1024 + 5), g4 = lit_at(14 * 1024 + 5);
    sc.fit(2 * 1024, 4 * 1024, g1, 0xFFFFFFFEull);
    sc.fit(6 * 1024, 7 * 1024, g2, 0xFFFFFFFEull);
    sc.fit(10 * 1024, 12 * 1024, g3, 0xFFFFFFFFull);
    sc.fit(14 * 1024, 15 * 1024, g4, 0xFFFFFFFFull);
    sc.len[lit_at(18 * 1024 + 5)] = 1ull << 33;
    sc.len[lit_at(18 * 1024 + 500)] = 1ull << 31;
    sc.len[lit_at(19 * 1024 + 7)] = 1ull << 32;
    sc.len[lit_at(19 * 1024 + 900)] = 1ull << 33;
    sc.need_wide = sc.need_exact = sc.need_mixed = true;
    return sc;
}
SmScn sm_scn_limit32(uint64_t seed) {
    SmScn sc = sm_scn_random("32-bit limit", 3 * 2048 + 11, seed);
    sc.idx_only = 4;
    uint64_t g = 2048 + 5;
    while (sc.sym[g] == kSelfTake) g++;
    sc.fit(0, sc.len.size(), g, kIdx32Limit - 1);       // the longest text load() gives the 32-bit engine
    sc.need_mixed = true;
    return sc;
}

static constexpr uint8_t kSmPoison = 0xA5;
template <class IDX>
struct SmDevice {
    grl32::DBuf<SelfRank> kinds, tstarts;
    grl32::DBuf<uint32_t> pre_sym, cell_sym, esym;
    grl32::DBuf<IDX> pre_len, cell_len, epos;
    uint64_t G = 0, Re = 0, queued = 0;
    SelfSeg<IDX> seg;
    void upload(const SmScn &sc, const SmRef &R) {
        G = sc.sym.size(); Re = sc.tsym.size();
        std::vector<uint64_t> kw(G / 64 + 1, 0), tw(R.take_total / 64 + 1, 0);      // (one word more than the bits need: ranks at the end of an axis read it)
        std::vector<uint32_t> ps, cs;
        std::vector<IDX> pl, cl, ep;
        for (uint64_t g = 0; g < G; g++) {
            if (sc.pre[g]) { kw[g >> 6] |= 1ull << (g & 63); ps.push_back(sc.sym[g]); pl.push_back((IDX)sc.len[g]); }
            else { cs.push_back(sc.sym[g]); cl.push_back((IDX)sc.len[g]); }
            if (R.inner[g] > 8) queued++;
        }
        uint64_t x = 0;
        for (uint64_t k = 0; k < Re; k++) { tw[x >> 6] |= 1ull << (x & 63); ep.push_back((IDX)x); x += sc.tlen[k]; }
        std::vector<uint32_t> es = sc.tsym;
        if (ps.empty()) { ps.push_back(0); pl.push_back(0); }
        if (cs.empty()) { cs.push_back(0); cl.push_back(0); }
        if (es.empty()) { es.push_back(0); ep.push_back(0); }
        self_upload(kinds, self_rank_cells(kw)); self_upload(tstarts, self_rank_cells(tw));
        self_upload(pre_sym, ps); self_upload(pre_len, pl); self_upload(cell_sym, cs); self_upload(cell_len, cl);
        self_upload(esym, es); self_upload(epos, ep);
        seg = SelfSeg<IDX>{kinds.p, pre_sym.p, pre_len.p, cell_sym.p, cell_len.p, kSelfTake, tstarts.p, esym.p, epos.p};
    }
};
// 0, or 3: a total differs, 4: a run differs, 5: an entry behind the runs was written
template <class IDX>
int sm_compare(const SmScn &sc, const SmRef &R, int spt, const char *form, const prim::SmPlan<IDX> &plan, const grl32::DBuf<uint32_t> &osym,
               const grl32::DBuf<IDX> &ostart, bool arrays) {
    const int ib = (int)sizeof(IDX);
    if (plan.take_total != R.take_total || plan.len_total != R.len_total || plan.heads != R.rsym.size() || plan.atoms != R.atoms) {
        fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, %s: totals (TAKE symbols, symbols, runs, atoms) "
                "expected (%llu, %llu, %llu, %llu), got (%llu, %llu, %llu, %llu)\n", sc.name, ib, spt, form,
                (unsigned long long)R.take_total, (unsigned long long)R.len_total, (unsigned long long)R.rsym.size(), (unsigned long long)R.atoms,
                (unsigned long long)plan.take_total, (unsigned long long)plan.len_total, (unsigned long long)plan.heads, (unsigned long long)plan.atoms);
        return 3;
    }
    if (!arrays) return 0;
    const std::vector<uint32_t> hs = osym.to_host(osym.n);
    const std::vector<IDX> hp = ostart.to_host(ostart.n);
    const uint64_t heads = R.rsym.size();
    for (uint64_t k = 0; k < heads; k++) {
        if (hs[k] != R.rsym[k] || hp[k] != (IDX)R.rstart[k]) {
            fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, %s: run %llu of %llu expected (symbol %u, start %llu), "
                    "got (%u, %llu)\n", sc.name, ib, spt, form, (unsigned long long)k, (unsigned long long)heads, R.rsym[k], (unsigned long long)R.rstart[k],
                    hs[k], (unsigned long long)hp[k]);
            return 4;
        }
    }
    IDX poison;
    memset(&poison, kSmPoison, sizeof(IDX));
    for (uint64_t k = heads; k < osym.n; k++) {
        if (hs[k] != 0xA5A5A5A5u || hp[k] != poison) {
            fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, %s: entry %llu behind the %llu runs was written: "
                    "(%u, %llu)\n", sc.name, ib, spt, form, (unsigned long long)k, (unsigned long long)heads, hs[k], (unsigned long long)hp[k]);
            return 5;
        }
    }
    return 0;
}
template <class IDX>
void sm_poison(grl32::DBuf<uint32_t> &osym, grl32::DBuf<IDX> &ostart, uint64_t n) {
    osym.alloc(n); ostart.alloc(n);
    prim::dev_memset(osym.p, kSmPoison, n * sizeof(uint32_t));
    prim::dev_memset(ostart.p, kSmPoison, n * sizeof(IDX));
}
// count + emit; the totals are compared before the emit pass runs (its arrays are sized from the reference)
template <class IDX>
int sm_two_pass(const SmScn &sc, const SmRef &R, const SmDevice<IDX> &D, bool mostly_plain, const char *form) {
    const int spt = mostly_plain ? 4 : 8;
    prim::SmPlan<IDX> plan;
    grl32::DBuf<uint32_t> osym;
    grl32::DBuf<IDX> ostart;
    int rc = 0;
    try {
        prim::stream_merge_count<SelfSeg<IDX>, IDX>(D.G, D.seg, plan, "selftest.sm", mostly_plain);
        rc = sm_compare<IDX>(sc, R, spt, form, plan, osym, ostart, false);
        if (!rc) {
            sm_poison<IDX>(osym, ostart, R.rsym.size() + 64);
            prim::stream_merge_emit<SelfSeg<IDX>, IDX>(D.seg, plan, osym.p, ostart.p, "selftest.sm");
            rc = sm_compare<IDX>(sc, R, spt, form, plan, osym, ostart, true);
        }
    } catch (...) { plan.release(); throw; }
    plan.release();
    return rc;
}
// the one walk.  how: 0 = as the engine calls it, 1 = a queue one entry short (must give up), 2 = no patience (may give up)
template <class IDX>
int sm_one_walk(const SmScn &sc, const SmRef &R, const SmDevice<IDX> &D, bool mostly_plain, int how) {
    const int spt = mostly_plain ? 4 : 8;
    const char *form = how == 0 ? "one walk" : (how == 1 ? "one walk, queue one entry short" : "one walk, no patience");
    const uint64_t cap = D.G + D.Re + 1;      // (an upper bound of the runs: the kernel does not bound its stores by it)
    prim::SmPlan<IDX> plan;
    grl32::DBuf<uint32_t> osym;
    grl32::DBuf<IDX> ostart;
    sm_poison<IDX>(osym, ostart, cap);
    int rc = 0;
    bool done = false;
    try {
        const uint64_t qcap = how == 1 ? D.queued - 1 : D.queued;
        // (the fall-backs run on the device only, so the patience goes to the device library alone: the serial walk waits for nobody)
#ifdef GRLBWT_PRIM_HIP
        if (how == 2) done = prim::stream_merge_onepass<SelfSeg<IDX>, IDX>(D.G, D.seg, plan, osym.p, ostart.p, cap, qcap, "selftest.sm1", mostly_plain, (uint64_t)0);
        else
#endif
        done = prim::stream_merge_onepass<SelfSeg<IDX>, IDX>(D.G, D.seg, plan, osym.p, ostart.p, cap, qcap, "selftest.sm1", mostly_plain);
        if (done) {
            if (how == 1) {
                fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, %s: the walk did not give up\n", sc.name, (int)sizeof(IDX), spt, form);
                rc = 7;
            } else rc = sm_compare<IDX>(sc, R, spt, form, plan, osym, ostart, true);
        }
    } catch (...) { plan.release(); throw; }
    if (!done) {
        // gave up: the plan holds nothing but G, and count + emit give the result
        bool empty = plan.G == D.G && plan.heads == 0 && plan.atoms == 0 && plan.take_total == 0 && plan.len_total == 0;
        if constexpr (prim::kIsDevice) empty = empty && !plan.xbase && !plan.lbase && !plan.hbase && !plan.tlast;
        const uint64_t tiles = (D.G + 256ull * spt - 1) / (256ull * spt);
        if (!empty) {
            fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, %s: gave up and left a plan behind\n", sc.name, (int)sizeof(IDX), spt, form);
            rc = 7;
        } else if (prim::kIsDevice && how == 0 && tiles <= 256) {      // (every tile resident at once: nobody waits for a tile that has not started)
            fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, %s: gave up in a grid of %llu tiles\n", sc.name, (int)sizeof(IDX), spt, form,
                    (unsigned long long)tiles);
            rc = 6;
        } else {
            if (how == 0) fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread: 1 give-up at the default patience in a grid of %llu tiles\n",
                                  sc.name, (int)sizeof(IDX), spt, (unsigned long long)tiles);
            plan.release();
            rc = sm_two_pass<IDX>(sc, R, D, mostly_plain, how == 0 ? "count + emit behind a give-up" : (how == 1 ? "count + emit behind a full queue" : "count + emit behind no patience"));
        }
    }
    plan.release();
    return rc;
}
// count + emit records (device library only): run k as the low 1 + fb bytes of (symbol | length << 8), the symbol as it is or through a
// table; `out` at 0, 1, 5 and 15 bytes behind a 16-byte boundary, poisoned bytes on both sides.  (A length wider than fb bytes loses
// its top on both sides of the comparison; the scenario with 2^33-symbol runs takes only the widths that hold them.)
#ifdef GRLBWT_PRIM_HIP
struct SelfRecFn {
    const uint64_t *table;
    GRL_DEV uint64_t operator()(uint32_t sym, uint64_t len) const { return (table ? table[sym & 3u] : (uint64_t)(sym & 0xFFu)) | (len << 8); }
};
template <class IDX>
int sm_records(const SmScn &sc, const SmRef &R, const SmDevice<IDX> &D, bool mostly_plain) {
    static const uint32_t kFb[3] = {1, 4, 7}, kOff[4] = {0, 1, 5, 15};
    static const std::vector<uint64_t> kTable = {0x11, 0x22, 0x33, 0x44};
    const int spt = mostly_plain ? 4 : 8;
    const uint64_t heads = R.rsym.size(), guard = 48;
    prim::SmPlan<IDX> plan;
    grl32::DBuf<uint32_t> none32;
    grl32::DBuf<IDX> none;
    grl32::DBuf<uint64_t> table;
    grl32::DBuf<uint8_t> buf;
    self_upload(table, kTable);
    int rc = 0;
    try {
        prim::stream_merge_count<SelfSeg<IDX>, IDX>(D.G, D.seg, plan, "selftest.sm", mostly_plain);
        rc = sm_compare<IDX>(sc, R, spt, "count + emit records", plan, none32, none, false);
        for (int f = 0; f < 3 && !rc; f++) {
            const uint32_t fb = kFb[f], rec = 1 + fb;
            if (sc.need_wide && fb < 5) continue;
            for (int tab = 0; tab < 2 && !rc; tab++)
                for (int o = 0; o < 4 && !rc; o++) {
                    const uint64_t bytes = heads * rec, cap = 16 + guard + bytes + guard;
                    buf.alloc(cap);
                    prim::dev_memset(buf.p, kSmPoison, cap);
                    const uint64_t at = (16 - ((uintptr_t)buf.p & 15)) % 16 + 16 + kOff[o];      // (>= 16 poisoned bytes in front, >= guard behind)
                    prim::stream_merge_emit_records<SelfSeg<IDX>, IDX>(D.seg, plan, buf.p + at, rec, SelfRecFn{tab ? table.p : nullptr}, "selftest.sm");
                    const std::vector<uint8_t> h = buf.to_host(cap);
                    for (uint64_t k = 0; k < heads && !rc; k++) {
                        const uint64_t len = (k + 1 < heads ? R.rstart[k + 1] : R.len_total) - R.rstart[k];
                        const uint64_t v = (tab ? kTable[R.rsym[k] & 3u] : (uint64_t)(R.rsym[k] & 0xFFu)) | (len << 8);
                        uint64_t got = 0;
                        for (uint32_t b = 0; b < rec; b++) got |= (uint64_t)h[at + k * rec + b] << (8 * b);
                        if (got != (rec < 8 ? v & ((1ull << (8 * rec)) - 1ull) : v)) {
                            fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, records of 1 + %u bytes%s at offset %u: "
                                    "record %llu of %llu expected %llx (symbol %u, length %llu), got %llx\n", sc.name, (int)sizeof(IDX), spt, fb, tab ? " through a table" : "", kOff[o],
                                    (unsigned long long)k, (unsigned long long)heads, (unsigned long long)v, R.rsym[k], (unsigned long long)len, (unsigned long long)got);
                            rc = 8;
                        }
                    }
                    for (uint64_t x = 0; x < cap && !rc; x++) {
                        if ((x < at || x >= at + bytes) && h[x] != kSmPoison) {
                            fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread, records of 1 + %u bytes at offset %u: "
                                    "byte %lld %s the records was written\n", sc.name, (int)sizeof(IDX), spt, fb, kOff[o],
                                    x < at ? (long long)(at - x) : (long long)(x - (at + bytes)), x < at ? "in front of" : "behind");
                            rc = 9;
                        }
                    }
                }
        }
    } catch (...) { plan.release(); throw; }
    plan.release();
    return rc;
}
#endif
template <class IDX>
int sm_check(const SmScn &sc, const SmRef &R, bool fallbacks) {
    if (sc.idx_only && sc.idx_only != (int)sizeof(IDX)) return 0;
    SmDevice<IDX> D;
    D.upload(sc, R);
    for (int mp = 0; mp < 2; mp++) {
        if (int rc = sm_two_pass<IDX>(sc, R, D, mp != 0, "count + emit")) return 200 + rc;
        if (int rc = sm_one_walk<IDX>(sc, R, D, mp != 0, 0)) return 210 + rc;
        if (prim::kIsDevice && fallbacks) {
            if (D.queued) if (int rc = sm_one_walk<IDX>(sc, R, D, mp != 0, 1)) return 220 + rc;
            if (int rc = sm_one_walk<IDX>(sc, R, D, mp != 0, 2)) return 230 + rc;
        }
#ifdef GRLBWT_PRIM_HIP
        if (int rc = sm_records<IDX>(sc, R, D, mp != 0)) return 240 + rc;
#endif
    }
    return 0;
}
int test_stream_merge(uint64_t n, uint64_t seed) {
    SmScn scn[6] = {sm_scn_mix(self_size(n), seed + 20), sm_scn_one_run(seed + 21), sm_scn_seam(seed + 22), sm_scn_wide(seed + 23), sm_scn_wide64(seed + 24),
                    sm_scn_limit32(seed + 25)};
    for (SmScn &sc : scn) {
        SmRef R;
        sm_reference(sc, R);
        uint64_t tt = 0;
        for (uint64_t l : sc.tlen) tt += l;
        if (tt != R.take_total) return -202;
        if (R.len_total <= ((uint64_t)1 << 24) && !sm_reference_agrees_with_expansion(sc, R)) {
            fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s': the reference walk and the expanded string disagree\n", sc.name);
            return -202;
        }
        for (int spt = 4; spt <= 8; spt += 4)
            for (int ib = 4; ib <= 8; ib += 4) {
                if (sc.idx_only && sc.idx_only != ib) continue;
                if (const char *lost = sm_scenario_lost(sc, R, spt, ib)) {
                    fprintf(stderr, "[grlbwt] selftest stream merge: scenario '%s', %d-byte index, %d segments per thread: the input has no %s\n", sc.name, ib, spt, lost);
                    return -201;
                }
            }
        const bool fallbacks = sc.need_queued || sc.need_plain || sc.need_zero;      // (wide, mix at its full size, one run)
        if (int rc = sm_check<uint32_t>(sc, R, fallbacks)) return -rc;
        if (int rc = sm_check<uint64_t>(sc, R, fallbacks)) return -(rc + 40);
    }
    return 0;
}

// ---- 2: groups ordered in LDS (device library only: the stand-in has no such primitive)
#ifdef GRLBWT_PRIM_HIP
struct SelfSegSortFn {
    const uint32_t *bounds; const uint64_t *keys; uint32_t *src; uint64_t *okey; uint8_t *flag; uint32_t *hits;
    GRL_DEV uint32_t begin(uint64_t b) const { return bounds[2 * b]; }
    GRL_DEV uint32_t end(uint64_t b) const { return bounds[2 * b + 1]; }
    GRL_DEV uint64_t key(uint32_t i) const { return keys[i]; }
    GRL_DEV void write(uint32_t pos, uint32_t item, uint64_t k, bool first, bool beside) const {
        src[pos] = item; okey[pos] = k; flag[pos] = (uint8_t)((first ? 1 : 0) | (beside ? 2 : 0));
        atomicAdd(&hits[pos], 1u);
    }
};
// groups of the sizes in (lo, hi] (and of 2 and 3 items, shorter than the padded length the launch allows), four kinds of keys each
template <int TB>
int test_seg_sort(const std::vector<uint32_t> &sizes, uint32_t lo, uint32_t hi, uint64_t seed) {
    static constexpr uint32_t kGap = 5;
    std::vector<uint32_t> bounds;
    std::vector<uint64_t> keys;
    uint64_t s = seed;
    for (uint32_t sz : sizes) {
        if (!((sz > lo && sz <= hi) || sz <= 3)) continue;
        for (int kind = 0; kind < 4; kind++) {
            for (uint32_t g = 0; g < kGap; g++) keys.push_back(0);
            bounds.push_back((uint32_t)keys.size());
            const uint64_t salt = sm64(s), run = 1 + sm64(s) % 7;
            for (uint32_t i = 0; i < sz; i++) {
                uint64_t k;
                if (kind == 0) k = self_mix(salt + i);                                  // all distinct (the mix is a bijection)
                else if (kind == 1) k = salt;                                           // all equal
                else if (kind == 2) k = self_mix(salt + i / run) % 97;                 // runs of duplicates, and duplicates apart
                else k = (self_mix(salt + i) % 3 == 0) ? ~0ull : self_mix(salt + i) % 5;      // the padding key among the keys
                keys.push_back(k);
            }
            bounds.push_back((uint32_t)keys.size());
        }
    }
    for (uint32_t g = 0; g < kGap; g++) keys.push_back(0);
    const uint64_t N = keys.size(), nseg = bounds.size() / 2;
    grl32::DBuf<uint32_t> db, dsrc(N), dhits(N);
    grl32::DBuf<uint64_t> dk, dok(N);
    grl32::DBuf<uint8_t> dfl(N);
    self_upload(db, bounds); self_upload(dk, keys);
    prim::dev_memset(dsrc.p, 0xA5, N * 4); prim::dev_memset(dok.p, 0xA5, N * 8); prim::dev_memset(dfl.p, 0xA5, N); dhits.zero();
    try {
        prim::seg_sort_lds<TB>(nseg, SelfSegSortFn{db.p, dk.p, dsrc.p, dok.p, dfl.p, dhits.p}, hi, "selftest.seg_sort");
        prim::sync();
    } catch (const prim::Error &e) {
        fprintf(stderr, "[grlbwt] selftest seg_sort_lds: %d threads, groups of up to %u items: %s\n", TB, hi, e.what());
        return 1;
    }
    const std::vector<uint32_t> hsrc = dsrc.to_host(N), hhits = dhits.to_host(N);
    const std::vector<uint64_t> hok = dok.to_host(N);
    const std::vector<uint8_t> hfl = dfl.to_host(N);
    std::vector<uint8_t> covered(N, 0);
    std::vector<uint32_t> ord;
    for (uint64_t b = 0; b < nseg; b++) {
        const uint32_t a = bounds[2 * b], e = bounds[2 * b + 1], sz = e - a;
        ord.resize(sz);
        for (uint32_t i = 0; i < sz; i++) ord[i] = a + i;
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
        for (uint32_t p = 0; p < sz; p++) {
            const uint64_t k = keys[ord[p]];
            const bool eq_prev = p > 0 && keys[ord[p - 1]] == k, eq_next = p + 1 < sz && keys[ord[p + 1]] == k;
            const uint8_t fl = (uint8_t)(((p > 0 && !eq_prev) ? 1 : 0) | ((eq_prev || eq_next) ? 2 : 0));
            covered[a + p] = 1;
            int bad = 0;
            if (hsrc[a + p] != ord[p]) bad = 2; else if (hok[a + p] != k) bad = 3; else if (hfl[a + p] != fl) bad = 4; else if (hhits[a + p] != 1) bad = 5;
            if (bad) {
                fprintf(stderr, "[grlbwt] selftest seg_sort_lds: %d threads, padded to %u, group %llu of %u items (keys of kind %llu), position %u: expected item %u key %llx flags %u, "
                        "got item %u key %llx flags %u, written %u times\n", TB, hi, (unsigned long long)b, sz, (unsigned long long)(b % 4), p, ord[p] - a, (unsigned long long)k, fl,
                        hsrc[a + p] - a, (unsigned long long)hok[a + p], hfl[a + p], hhits[a + p]);
                return bad;
            }
        }
    }
    for (uint64_t i = 0; i < N; i++)
        if (!covered[i] && (hsrc[i] != 0xA5A5A5A5u || hfl[i] != 0xA5 || hhits[i] != 0)) {
            fprintf(stderr, "[grlbwt] selftest seg_sort_lds: %d threads, padded to %u: entry %llu between the groups was written\n", TB, hi, (unsigned long long)i);
            return 6;
        }
    return 0;
}
int test_seg_sort_all(uint64_t seed) {
    const uint32_t mx = prim::seg_sort_lds_max();
    static bool said = false;
    if (!said) { said = true; fprintf(stderr, "[grlbwt] selftest: seg_sort_lds_max() = %u items, %u bytes of LDS per workgroup\n", mx, prim::rt().lds_bytes); }
    std::vector<uint32_t> sizes = {2, 3, 63, 64, 65, 255, 256, 257, mx};
    for (uint32_t p = 2; p <= mx; p <<= 1) { sizes.push_back(p - 1); sizes.push_back(p); if (p < mx) sizes.push_back(p + 1); }
    std::sort(sizes.begin(), sizes.end());
    sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
    sizes.erase(std::remove_if(sizes.begin(), sizes.end(), [](uint32_t v) { return v < 2; }), sizes.end());
    const uint32_t tiers[4] = {3, 256, 4096, mx};
    for (int t = 0; t < 3; t++) {
        if (tiers[t] >= tiers[t + 1]) continue;
        if (int rc = test_seg_sort<64>(sizes, tiers[t], tiers[t + 1], seed + t)) return -(300 + rc);
        if (int rc = test_seg_sort<256>(sizes, tiers[t], tiers[t + 1], seed + 10 + t)) return -(310 + rc);
    }
    return 0;
}
#endif

// ---- 3: fixed-width records
struct SelfPackFn {
    uint64_t salt;
    GRL_DEV uint64_t operator()(uint64_t i) const { return self_mix(salt ^ (i * 0x9E3779B97F4A7C15ull)); }      // (all 64 bits: the high bytes must be dropped)
};
int test_pack() {
    static const uint64_t ns[5] = {1, 1023, 1024, 1025, 3 * 1024 + 7};
    static const uint32_t offs[3] = {0, 1, 20};
    const size_t cap = 64 + 20 + (3 * 1024 + 7) * 8 + 64;
    grl32::DBuf<uint8_t> d(cap);
    if ((uintptr_t)d.p & 15) return -401;
    std::vector<uint8_t> poison(cap, 0xC3), want, got(cap);
    for (uint32_t rec = 1; rec <= 8; rec++)
        for (uint64_t n : ns)
            for (uint32_t off : offs) {
                const uint64_t salt = rec * 1000003ull + n * 31 + off;
                const size_t used = 64 + off + n * rec + 64;
                prim::h2d(d.p, poison.data(), cap);
                prim::pack_records(n, SelfPackFn{salt}, rec, d.p + 64 + off, "selftest.pack");
                prim::d2h(got.data(), d.p, cap);
                want = poison;
                for (uint64_t i = 0; i < n; i++) {
                    const uint64_t v = self_mix(salt ^ (i * 0x9E3779B97F4A7C15ull));
                    for (uint32_t b = 0; b < rec; b++) want[64 + off + i * rec + b] = (uint8_t)(v >> (8 * b));
                }
                for (size_t x = 0; x < cap; x++)
                    if (got[x] != want[x]) {
                        const long at = (long)x - 64 - (long)off;
                        fprintf(stderr, "[grlbwt] selftest pack_records: %u-byte records, n = %llu, output %u bytes behind a 16-byte boundary: byte %ld (%s) expected %02x, got %02x\n",
                                rec, (unsigned long long)n, off, at, at < 0 ? "guard in front" : (x >= used - 64 ? "guard behind" : "record bytes"), want[x], got[x]);
                        return at < 0 || x >= used - 64 ? -403 : -402;
                    }
            }
    return 0;
}

// ---- 4: a functor over the set bits
struct SelfBitFn {
    uint64_t *out; uint32_t *hits;
    GRL_DEV void operator()(uint64_t p, uint64_t ord) const { out[ord] = p; prim::atomic_add(&hits[ord], 1u); }
};
// span 0: through for_each_set_bit, which picks 4..64 words per wave from the vector's length and the device's size -- 4 for every
// vector of the bounded sizes here; the longer spans are the kernel itself, launched the way for_each_set_bit does (device library only)
template <class IDX>
int test_set_bits_one(uint64_t nbits, int kind, uint64_t seed, uint32_t span = 0) {
    static const char *kinds[5] = {"empty", "all ones", "one bit in three", "one bit in a thousand", "dense and empty stretches"};
    const uint64_t nw = (nbits + 63) / 64;
    std::vector<uint64_t> words(nw, 0), pos;
    uint64_t s = seed;
    for (uint64_t p = 0; p < nbits; p++) {
        bool b = false;
        if (kind == 1) b = true;
        else if (kind == 2) b = sm64(s) % 3 == 0;
        else if (kind == 3) b = sm64(s) % 1000 == 0;
        else if (kind == 4) b = (p / 4096) % 2 == 0 && p % 4096 != 0;      // 63 bits, then full words: the ring holds 127 entries at every word
        if (b) { words[p >> 6] |= 1ull << (p & 63); pos.push_back(p); }
    }
    std::vector<IDX> base(nw + 1);
    uint64_t c = 0;
    for (uint64_t w = 0; w < nw; w++) { base[w] = (IDX)c; c += (uint64_t)__builtin_popcountll(words[w]); }
    base[nw] = (IDX)c;
    const uint64_t cnt = pos.size(), cap = cnt + 64;
    grl32::DBuf<uint64_t> dw, dout(cap);
    grl32::DBuf<IDX> db;
    grl32::DBuf<uint32_t> dhits(cap);
    self_upload(dw, words); self_upload(db, base);
    prim::dev_memset(dout.p, 0xA5, cap * 8); dhits.zero();
    if (!span) prim::for_each_set_bit<IDX>(nbits, dw.p, db.p, SelfBitFn{dout.p, dhits.p}, "selftest.set_bits");
#ifdef GRLBWT_PRIM_HIP
    else {
        const uint64_t waves = (nw + span - 1) / span;
        hipLaunchKernelGGL((prim::k_for_each_set_bit<IDX, SelfBitFn>), dim3((unsigned)((waves + prim::kBlock / 64 - 1) / (prim::kBlock / 64))), dim3(prim::kBlock), 0,
                           prim::rt().stream, nw, (const uint64_t *)dw.p, (const IDX *)db.p, span, SelfBitFn{dout.p, dhits.p});
        prim::after_launch("selftest.set_bits");
    }
#endif
    const std::vector<uint64_t> ho = dout.to_host(cap);
    const std::vector<uint32_t> hh = dhits.to_host(cap);
    for (uint64_t k = 0; k < cap; k++) {
        const uint64_t want = k < cnt ? pos[k] : 0xA5A5A5A5A5A5A5A5ull;
        const uint32_t wh = k < cnt ? 1u : 0u;
        if (ho[k] != want || hh[k] != wh) {
            fprintf(stderr, "[grlbwt] selftest for_each_set_bit: %d-byte ranks, %llu bits, %s, span %u: ordinal %llu of %llu expected position %llu (%u calls), got %llu (%u calls)\n",
                    (int)sizeof(IDX), (unsigned long long)nbits, kinds[kind], span, (unsigned long long)k, (unsigned long long)cnt, (unsigned long long)want, wh, (unsigned long long)ho[k], hh[k]);
            return k < cnt ? (ho[k] != want ? 1 : 2) : 3;
        }
    }
    return 0;
}
int test_set_bits(uint64_t n, uint64_t seed) {
    const uint64_t sizes[7] = {1, 64, 65, 4095, 4096, 4097, self_size(n)};
    for (uint64_t nbits : sizes)
        for (int kind = 0; kind < 5; kind++) {
            if (int rc = test_set_bits_one<uint32_t>(nbits, kind, seed + kind)) return -(500 + rc);
            if (int rc = test_set_bits_one<uint64_t>(nbits, kind, seed + 7 + kind)) return -(510 + rc);
        }
#ifdef GRLBWT_PRIM_HIP
    for (uint32_t span = 8; span <= 64; span <<= 1)
        for (int kind = 2; kind <= 4; kind += 2) {
            if (int rc = test_set_bits_one<uint32_t>(sizes[6], kind, seed + 20 + kind, span)) return -(520 + rc);
            if (int rc = test_set_bits_one<uint64_t>(sizes[5], kind, seed + 30 + kind, span)) return -(530 + rc);
        }
#endif
    return 0;
}

// 12: one refinement round of the image merge (Image::MergeRound: the three round kernels on the device) against a host loop: flags
// in runs of up to 9000 rows and in coin flips (tiles fed from one image alone, slices that start at any byte), rank bytes below sigma
template <class E>
int test_merge_round_one(uint64_t n, uint64_t seed, uint32_t sigma, int ib) {
    std::vector<uint8_t> z(n), prev(n);
    uint64_t s = seed, na = 0, exp_changed = 0;
    for (uint64_t i = 0; i < n;) {
        const uint64_t kind = sm64(s) % 3;
        uint64_t len = kind == 0 ? 1 + sm64(s) % 9000 : 1 + sm64(s) % 300;
        const uint8_t bit = (uint8_t)(sm64(s) & 1);
        for (; len && i < n; len--, i++) z[i] = kind == 2 ? (uint8_t)(sm64(s) & 1) : bit;
    }
    for (uint64_t i = 0; i < n; i++) {
        na += z[i] == 0;
        prev[i] = sm64(s) % 11 == 0 ? (uint8_t)(z[i] ^ 1) : z[i];
        exp_changed += prev[i] != z[i];
    }
    const uint64_t nb = n - na;
    std::vector<uint8_t> ra(na), rb(nb), want(n);
    for (auto &v : ra) v = (uint8_t)(sm64(s) % sigma);
    for (auto &v : rb) v = (uint8_t)(sm64(s) % sigma);
    {   // the definition: a stable sort of the flags by the symbol each reads from its own image
        std::vector<uint8_t> key(n);
        std::vector<uint64_t> at(257, 0);
        uint64_t i = 0, j = 0;
        for (uint64_t p = 0; p < n; p++) { key[p] = z[p] ? rb[j++] : ra[i++]; at[key[p] + 1]++; }
        for (int c = 0; c < 256; c++) at[c + 1] += at[c];
        for (uint64_t p = 0; p < n; p++) want[at[key[p]]++] = z[p];
    }
    grl32::DBuf<uint8_t> dra(na + 16), drb(nb + 16), dz(n + 16), dp(n + 16), dout(n + 64);
    prim::h2d(dra.p, ra.data(), na); prim::h2d(drb.p, rb.data(), nb); prim::h2d(dz.p, z.data(), n); prim::h2d(dp.p, prev.data(), n);
    prim::dev_memset(dout.p, 0xA5, n + 64);
    typename E::MergeRound W;
    W.alloc(n);
    if (W.changed(dz.p, dp.p, na) != exp_changed) return 1;
    if (W.changed(dz.p, nullptr, na) != 0) return 2;
    W.step(dra.p, drb.p, dz.p, dout.p);
    prim::sync();
    const std::vector<uint8_t> got = dout.to_host(n + 64);
    for (uint64_t p = 0; p < n; p++)
        if (got[p] != want[p]) {
            fprintf(stderr, "[grlbwt] selftest merge round: %d-byte index, %llu rows (%llu of A), %u symbols: row %llu expected flag %u, got %u\n", ib,
                    (unsigned long long)n, (unsigned long long)na, sigma, (unsigned long long)p, want[p], got[p]);
            return 3;
        }
    for (uint64_t p = n; p < n + 64; p++) if (got[p] != 0xA5) return 4;
    return 0;
}
int test_merge_round(uint64_t n, uint64_t seed) {
    const uint64_t m = self_size(n);
    const uint32_t sigmas[3] = {2, 5, 256};
    for (int k = 0; k < 3; k++) {
        if (int rc = test_merge_round_one<grl32::Image>(m, seed + k, sigmas[k], 4)) return -(600 + rc);
        if (int rc = test_merge_round_one<grl64::Image>(m + 1 + k, seed + 10 + k, sigmas[k], 8)) return -(610 + rc);
    }
    return 0;
}

// 13: the scan in two phases (SplitScan: total first, consumer second) against exclusive_scan + for_each, at the edges of a scan
// tile and of the second level of tile sums, whatever n the caller gave; no flag set, every flag set, coin flips
struct SelfSplitRefFn {
    const uint8_t *f; const uint32_t *ex; uint32_t *pos;
    GRL_DEV void operator()(uint64_t i) const { if (f[i]) pos[ex[i]] = (uint32_t)i; }
};
struct SelfSplitEmitFn {
    static constexpr bool kWaveEmit = false;
    uint32_t *pre; uint32_t *pos;
    GRL_DEV void operator()(uint64_t i, uint32_t ex, uint32_t v) const { pre[i] = ex; if (v) pos[ex] = (uint32_t)i; }
};
int test_split_scan(uint64_t seed) {
    const uint64_t tile = 2048, sizes[7] = {1, tile - 1, tile, tile + 1, tile * tile - 1, tile * tile, tile * tile + 1};
    for (int si = 0; si < 7; si++)
        for (int density = 0; density < 3; density++) {
            const uint64_t n = sizes[si];
            std::vector<uint8_t> f(n);
            uint64_t s = seed + 3 * si + density, want = 0;
            for (uint64_t i = 0; i < n; i++) { f[i] = density == 0 ? 0 : density == 1 ? 1 : (uint8_t)(sm64(s) % 3 == 0); want += f[i]; }
            grl32::DBuf<uint8_t> df(n);
            prim::h2d(df.p, f.data(), n);
            grl32::DBuf<uint32_t> ex(n + 1), ref(want + 1), pre(n), pos(want + 1);
            prim::dev_memset(ref.p, 0xA5, (want + 1) * 4); prim::dev_memset(pos.p, 0xA5, (want + 1) * 4);
            const uint32_t tot = prim::exclusive_scan<uint32_t>(n, grl32::ByteIn{df.p}, ex.p, false, "selftest.split_ref");
            prim::for_each(n, SelfSplitRefFn{df.p, ex.p, ref.p}, "selftest.split_ref");
            grl32::SplitScan<uint32_t, grl32::ByteIn> sc(n, grl32::ByteIn{df.p}, "selftest.split_scan");
            if (sc.total != want || tot != want) {
                fprintf(stderr, "[grlbwt] selftest split scan: n = %llu, density %d: total %llu, exclusive_scan %llu, expected %llu\n", (unsigned long long)n, density,
                        (unsigned long long)sc.total, (unsigned long long)tot, (unsigned long long)want);
                return 1;
            }
            sc.emit(SelfSplitEmitFn{pre.p, pos.p}, "selftest.split_scan");
            prim::sync();
            const std::vector<uint32_t> hex = ex.to_host(n), hpre = pre.to_host(n), href = ref.to_host(want + 1), hpos = pos.to_host(want + 1);
            for (uint64_t i = 0; i < n; i++)
                if (hpre[i] != hex[i]) {
                    fprintf(stderr, "[grlbwt] selftest split scan: n = %llu, density %d: element %llu got prefix %u, exclusive_scan gave %u\n", (unsigned long long)n,
                            density, (unsigned long long)i, hpre[i], hex[i]);
                    return 2;
                }
            for (uint64_t k = 0; k <= want; k++) if (hpos[k] != href[k]) return 3;
            if (hpos[want] != 0xA5A5A5A5u) return 4;
        }
    return 0;
}

int selftest(uint64_t n, uint64_t seed) {
    if (n < 2) n = 2;
    std::vector<uint32_t> h(n);
    uint64_t s = seed;
    for (uint64_t i = 0; i < n; i++) h[i] = (uint32_t)sm64(s);
    grl32::DBuf<uint32_t> d(n);
    prim::h2d(d.p, h.data(), n * 4);
    // 1: exclusive scan (u64) with total
    {
        grl32::DBuf<uint64_t> o(n + 1);
        uint64_t tot = prim::exclusive_scan<uint64_t>(n, U32In{d.p}, o.p, true, "selftest.scan");
        auto ho = o.to_host(n + 1);
        uint64_t acc = 0;
        for (uint64_t i = 0; i < n; i++) { if (ho[i] != acc) return -1; acc += h[i] & 1023u; }
        if (ho[n] != acc || tot != acc) return -2;
    }
    // 2: exclusive scan (u32), in place over a pointer input
    {
        std::vector<uint32_t> small(n);
        for (uint64_t i = 0; i < n; i++) small[i] = h[i] & 7u;
        grl32::DBuf<uint32_t> o(n);
        prim::h2d(o.p, small.data(), n * 4);
        uint32_t tot = prim::exclusive_scan<uint32_t>(n, prim::PtrIn<uint32_t>{o.p}, o.p, false, "selftest.scan32");
        auto ho = o.to_host(n);
        uint32_t acc = 0;
        for (uint64_t i = 0; i < n; i++) { if (ho[i] != acc) return -3; acc += small[i]; }
        if (tot != acc) return -4;
    }
    // 3: reductions
    {
        uint64_t sum = 0; uint32_t mn = ~0u, mx = 0;
        for (uint64_t i = 0; i < n; i++) { sum += h[i] & 1023u; if (h[i] < mn) mn = h[i]; if (h[i] > mx) mx = h[i]; }
        if (prim::reduce_sum<uint64_t>(n, U32In{d.p}) != sum) return -5;
        if (prim::reduce_min<uint32_t>(n, U32Raw{d.p}) != mn) return -6;
        if (prim::reduce_max<uint32_t>(n, U32Raw{d.p}) != mx) return -7;
    }
    // 4: ballot bit-vector
    {
        uint64_t nw = (n + 63) / 64;
        grl32::DBuf<uint64_t> w(nw);
        prim::bitvector_from_pred(n, OddPred{d.p}, w.p, "selftest.bits");
        auto hw = w.to_host(nw);
        for (uint64_t i = 0; i < n; i++) {
            bool b = (hw[i >> 6] >> (i & 63)) & 1ull;
            if (b != ((h[i] % 3u) == 1u)) return -8;
        }
        if (n % 64) if (hw[nw - 1] >> (n % 64)) return -9;
    }
    // 5: byte histogram
    {
        uint64_t hist[256], ref[256] = {0};
        const uint8_t *hb = (const uint8_t *)h.data();
        uint64_t nb = n * 4 - 3;     // odd length: exercises the tail path
        for (uint64_t i = 0; i < nb; i++) ref[hb[i]]++;
        prim::byte_histogram((const uint8_t *)d.p, nb, hist);
        for (int i = 0; i < 256; i++) if (hist[i] != ref[i]) return -10;
    }
    // 6: stable radix sort, all key/value widths used by the engine
    { int r = test_sort<uint32_t, uint32_t>(n, seed + 1, 19); if (r) return -20 - r; }
    { int r = test_sort<uint64_t, uint32_t>(n, seed + 2, 45); if (r) return -30 - r; }
    { int r = test_sort<uint32_t, uint64_t>(n, seed + 3, 8); if (r) return -40 - r; }
    { int r = test_sort<uint64_t, uint32_t>(n, seed + 4, 3); if (r) return -50 - r; }   // heavy duplicates
    { int r = test_sort<uint64_t, uint64_t>(n, seed + 5, 33); if (r) return -60 - r; }
    { int r = test_sort_keys(n, seed + 6, 21); if (r) return -90 - r; }
    // digit plans with 9- and 10-bit digits (GRLBWT_SORT_DIGIT): 54 = 6 x 9, 51 = 9,9,9,8,8,8, 18 = 9,9, 27 = 9,9,9, 20 = 10,10
    { int r = test_sort<uint64_t, uint32_t>(n, seed + 7, 54); if (r) return -100 - r; }
    { int r = test_sort<uint64_t, uint32_t>(n, seed + 8, 51); if (r) return -110 - r; }
    { int r = test_sort_keys(n, seed + 9, 18); if (r) return -120 - r; }
    { int r = test_sort<uint32_t, uint64_t>(n, seed + 10, 27); if (r) return -130 - r; }
    { int r = test_sort<uint32_t, uint32_t>(n, seed + 11, 20); if (r) return -140 - r; }
    // 6b: partition sort that can be undone + per-partition de-duplication (the phrase naming of the levels above 0)
    { int r = test_part(n, seed + 12, 6); if (r) return -150 - r; }
    { int r = test_part(n, seed + 13, 11); if (r) return -160 - r; }
    { int r = test_part(n, seed + 14, 18); if (r) return -170 - r; }
    // 7: fused pair scans (8- and 16-byte elements: the 16-byte result stores and the LDS staging of the scan)
    { int r = test_pair_scan<uint32_t, uint32_t>(n, h, d.p); if (r) return -70 - r; }
    { int r = test_pair_scan<uint64_t, uint64_t>(n, h, d.p); if (r) return -80 - r; }
    // 8-11: what only whole builds reached (sizes taken from n are capped: see self_size)
    { int r = test_stream_merge(n, seed); if (r) return r; }
#ifdef GRLBWT_PRIM_HIP
    { int r = test_seg_sort_all(seed + 40); if (r) return r; }
#endif
    { int r = test_pack(); if (r) return r; }
    { int r = test_set_bits(n, seed + 60); if (r) return r; }
    { int r = test_merge_round(n, seed + 80); if (r) return r; }
    { int r = test_split_scan(seed + 90); if (r) return -(700 + r); }
    return 0;
}

}   // namespace

extern "C" {

int grlbwt_abi_version(void) { return GRLBWT_ABI_VERSION; }
const char *grlbwt_backend_name(void) { return prim::kIsDevice ? "hip-gfx950" : "serial-test-standin"; }

const char *grlbwt_strerror(int code) {
    switch (code) {
        case GRLBWT_OK: return "ok";
        case GRLBWT_EINVAL: return "invalid argument or call out of order";
        case GRLBWT_EDEVICE: return "HIP device/runtime error";
        case GRLBWT_ENOMEM: return "out of memory";
        case GRLBWT_EILLFORMED: return "Error: the file is ill formed";
        case GRLBWT_ERANGE: return "input beyond the supported range";
        case GRLBWT_ENOSPC: return "phrase table overflow";
        case GRLBWT_EINTERNAL: return "internal consistency check failed";
        case GRLBWT_ENOTDNA: return "The input seems not to be DNA";
        default: return "unknown error";
    }
}
const char *grlbwt_last_error(const grlbwt_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

// The GRLBWT_* environment switches choose between forms of one computation (tests force most of them and compare the image
// with the oracle: none changes the output) -- but several change what a run COSTS by integer factors (GRLBWT_NOPOOL,
// GRLBWT_NO_PART, GRLBWT_DIST_REPLICATED_*).  A run that has any of them set says so, once per process, on stderr.
// (GRLBWT_QUIET_ENV=1 silences the note: the test suites set switches on purpose.)  Named are the variables of switches.hpp.
static void warn_env_switches_once() {
    static bool done = false;
    if (done) return;
    done = true;
    if (prim::sw().quiet_env) return;
    extern char **environ;
    std::string names;
    int n = 0;
    for (char **e = environ; e && *e; e++) {
        const char *eq = strchr(*e, '=');
        const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
        bool known = false;
        prim::Switches::for_each_name([&](const char *sw_name) { known = known || name == sw_name; });
        if (known) names += (n++ ? ", " : "") + name;
    }
    if (n) fprintf(stderr, "[grlbwt] note: %d GRLBWT_* switch%s set in the environment (%s): the image is the same, time and memory of this run may not be\n",
                   n, n == 1 ? "" : "es", names.c_str());
}

int grlbwt_ctx_create(int device_id, uint32_t flags, grlbwt_ctx **out) {
    if (!out) return GRLBWT_EINVAL;
    *out = nullptr;
    grlbwt_ctx *c = new (std::nothrow) grlbwt_ctx();
    if (!c) return GRLBWT_ENOMEM;
    c->flags = flags;
    c->device = device_id;
    int rc = guarded(c, [&] {
        warn_env_switches_once();
        prim::init(device_id);            // refuses a second device while contexts are alive (one GPU per process)
        if (flags & GRLBWT_FLAG_CLASSIC_POOL) prim::pool_classic();
        if (flags & GRLBWT_FLAG_SYNC_DEBUG) prim::rt().sync_each_launch = true;
        prim::rt().live_ctx++;
    });
    if (rc != GRLBWT_OK) { delete c; return rc; }
    *out = c;
    return GRLBWT_OK;
}
void grlbwt_ctx_destroy(grlbwt_ctx *ctx) {
    if (!ctx) return;
    try {
        for (grlbwt_fm *fm : ctx->fms) delete fm;
        ctx->fms.clear();
        for (grlbwt_merge *mg : ctx->merges) delete mg;
        ctx->merges.clear();
        for (grlbwt_select *sel : ctx->selects) delete sel;
        ctx->selects.clear();
        for (grlbwt_docs *dc : ctx->docs) delete dc;
        ctx->docs.clear();
        for (grlbwt_debruijn *g : ctx->graphs) delete g;
        ctx->graphs.clear();
        for (grlbwt_cdebruijn *g : ctx->cgraphs) delete g;
        ctx->cgraphs.clear();
        ctx->e32.reset(); ctx->e64.reset(); prim::sync(); prim::pool_trim();
        if (--prim::rt().live_ctx <= 0) {      // process-wide debug settings and a borrowed stream end with the last context
            prim::rt().live_ctx = 0;
            prim::rt().sync_each_launch = false;
            prim::set_stream(nullptr);
        }
    } catch (...) {}
    delete ctx;
}
int grlbwt_ctx_set_stream(grlbwt_ctx *ctx, void *hip_stream) {
    if (!ctx) return GRLBWT_EINVAL;
    return guarded(ctx, [&] { prim::sync(); prim::set_stream(hip_stream); });   // work queued on the old stream finishes first
}

int grlbwt_text_upload(grlbwt_ctx *ctx, const void *host_cells, uint64_t n_cells, int cell_bytes) {
    if (!ctx || !host_cells) return refuse(ctx);
    return guarded(ctx, [&] { load(ctx, host_cells, n_cells, cell_bytes, true); });
}
int grlbwt_text_load_file(grlbwt_ctx *ctx, const char *path, int cell_bytes) {
    if (!ctx || !path) return refuse(ctx);
    return guarded(ctx, [&] { load_file(ctx, path, cell_bytes); });
}
int grlbwt_text_load_file_range(grlbwt_ctx *ctx, const char *path, uint64_t offset_bytes, uint64_t n_bytes, int cell_bytes) {
    if (!ctx || !path) return refuse(ctx);
    return guarded(ctx, [&] { load_file(ctx, path, cell_bytes, offset_bytes, n_bytes); });
}
int grlbwt_fastx_probe(const char *path, int *is_fastx, int *is_gz) {
    if (!path) return GRLBWT_EINVAL;
    unsigned char mg[2];
    if (!file_magic(path, mg)) return GRLBWT_EINVAL;
    // check_gzip (external/cdt/lib/utils.cpp:53-60): extension ".gz" AND the magic number
    const std::string p(path);
    const bool gz = p.size() >= 3 && p.compare(p.size() - 3, 3, ".gz") == 0 && mg[0] == 0x1F && mg[1] == 0x8B;
    unsigned char first = mg[0];
    if (gz) {                                                        // is_fastx (utils.cpp:13-30): first DEcompressed byte
        gzFile z = gzopen(path, "rb");
        if (!z) return GRLBWT_EINVAL;
        first = 0;
        gzread(z, &first, 1);
        gzclose(z);
    }
    if (is_gz) *is_gz = gz ? 1 : 0;
    if (is_fastx) *is_fastx = (first == '>' || first == '@') ? 1 : 0;
    return GRLBWT_OK;
}
int grlbwt_fastx_convert_device(grlbwt_ctx *ctx, const void *dev_in, uint64_t n_in, uint32_t fx_flags, void *dev_out, uint64_t capacity,
                                uint64_t *n_out, uint64_t *n_strings) {
    if (!ctx || !dev_in || !dev_out) return refuse(ctx);
    return guarded(ctx, [&] {
        grl64::Engine::FastxInfo info = grl64::Engine::fastx_to_text((const uint8_t *)dev_in, n_in, (fx_flags & GRLBWT_FASTX_REVCOMP) != 0,
                                                                     (uint8_t *)dev_out, capacity);
        if (n_out) *n_out = info.n_out;
        if (n_strings) *n_strings = info.n_strings;
    });
}
int grlbwt_alphabet_size(const grlbwt_ctx *ctx, uint64_t *n_distinct) {
    if (!HAS_ENG(ctx) || !n_distinct) return refuse(ctx);
    *n_distinct = ENG(ctx, alpha_n);
    return GRLBWT_OK;
}
int grlbwt_alphabet_download(const grlbwt_ctx *ctx, uint64_t *values_out) {
    if (!HAS_ENG(ctx) || !values_out || ENG(ctx, alpha_n) == 0) return refuse(ctx);
    return guarded(const_cast<grlbwt_ctx *>(ctx), [&] { prim::d2h(values_out, ENG(ctx, alpha.p), ENG(ctx, alpha_n) * 8); });
}
int grlbwt_alphabet_compact_device(grlbwt_ctx *ctx, const void *dev_cells, uint64_t n_cells, int cell_bytes, void *dev_ranks_u32,
                                   void *dev_values_u64, uint64_t capacity_values, uint64_t *n_distinct) {
    if (!ctx || !dev_cells || !dev_ranks_u32 || !dev_values_u64 || n_cells == 0 || !(cell_bytes == 4 || cell_bytes == 8)) return refuse(ctx);
    return guarded(ctx, [&] {
        const bool big = idx64_for(ctx, n_cells);
        uint64_t k = big ? grl64::Engine::alphabet_compact_device(dev_cells, n_cells, cell_bytes, (uint32_t *)dev_ranks_u32, (uint64_t *)dev_values_u64, capacity_values)
                         : grl32::Engine::alphabet_compact_device(dev_cells, n_cells, cell_bytes, (uint32_t *)dev_ranks_u32, (uint64_t *)dev_values_u64, capacity_values);
        if (n_distinct) *n_distinct = k;
        if (k > capacity_values) throw prim::Error(GRLBWT_EINVAL, "alphabet compaction: more distinct values than the output buffer holds");
    });
}
int grlbwt_text_load_fastx(grlbwt_ctx *ctx, const char *path, uint32_t fx_flags, uint64_t *n_strings) {
    if (!ctx || !path) return refuse(ctx);
    return guarded(ctx, [&] { load_fastx(ctx, path, fx_flags, n_strings); });
}
int grlbwt_text_attach_device(grlbwt_ctx *ctx, const void *dev_cells, uint64_t n_cells, int cell_bytes) {
    if (!ctx || !dev_cells || ((uintptr_t)dev_cells & 15)) return refuse(ctx);
    return guarded(ctx, [&] { load(ctx, dev_cells, n_cells, cell_bytes, false); });
}
int grlbwt_get_stats(const grlbwt_ctx *ctx, grlbwt_stats *out) {
    if (!HAS_ENG(ctx)) return refuse(ctx, "no text is loaded in this context");
    if (!out) return refuse(ctx, "null argument");
    if (ctx->e32) fill_stats(*ctx->e32, out); else fill_stats(*ctx->e64, out);
    return GRLBWT_OK;
}

int grlbwt_parse_round(grlbwt_ctx *ctx, grlbwt_round_info *info, int *done) {
    return stage(ctx, nullptr, [&] {
        bool d = ENG(ctx, parse_round());
        if (done) *done = d ? 1 : 0;
        if (info) { int r = (int)ENG(ctx, levels.size()) - 1; if (ctx->e32) fill_round(*ctx->e32, r, info); else fill_round(*ctx->e64, r, info); }
    });
}
int grlbwt_parse_phase(grlbwt_ctx *ctx, int *n_rounds) {
    return stage(ctx, nullptr, [&] { int r = ENG(ctx, parse_phase()); if (n_rounds) *n_rounds = r; });
}
int grlbwt_round_info_get(const grlbwt_ctx *ctx, int round, grlbwt_round_info *info) {
    if (!HAS_ENG(ctx) || !info || round < 0 || round >= (int)ENG(ctx, levels.size())) return refuse(ctx);
    if (ctx->e32) fill_round(*ctx->e32, round, info); else fill_round(*ctx->e64, round, info);
    return GRLBWT_OK;
}

int grlbwt_induce_first(grlbwt_ctx *ctx) {
    const char *why = nullptr;
    if (HAS_ENG(ctx)) {
        if (!ENG(ctx, parse_done)) why = "parse phase not finished";
        else if (ENG(ctx, done())) why = "the image is built already: grlbwt_induce_first runs once per text";
        else if (ENG(ctx, bwt_level) >= 0) why = "the induction has begun already: grlbwt_induce_first runs once per text";
    }
    return stage(ctx, why, [&] { ENG(ctx, first_bwt()); });
}
int grlbwt_induce_level(grlbwt_ctx *ctx, int *level, grlbwt_level_info *info) {
    const char *why = nullptr;
    if (HAS_ENG(ctx)) {
        if (ENG(ctx, done())) why = "the image is built already: no level left to induce";
        else if (ENG(ctx, bwt_level) <= 0) why = "no level to induce: grlbwt_induce_first comes first";
    }
    return stage(ctx, why, [&] {
        ENG(ctx, induce_level());
        int l = ENG(ctx, bwt_level);
        if (level) *level = l;
        if (info) { if (ctx->e32) fill_level(*ctx->e32, l, info); else fill_level(*ctx->e64, l, info); }
        if (l == 0) ENG(ctx, finish());
    });
}
int grlbwt_induce_phase(grlbwt_ctx *ctx) {
    const char *why = HAS_ENG(ctx) && !ENG(ctx, parse_done) ? "parse phase not finished" : nullptr;
    return stage(ctx, why, [&] {
        if (ENG(ctx, done())) return;          // DONE: the image stands
        ENG(ctx, induce_phase());              // PARSED, or INDUCING: the levels that are left
        ENG(ctx, finish());
    });
}
int grlbwt_level_info_get(const grlbwt_ctx *ctx, int level, grlbwt_level_info *info) {
    if (!HAS_ENG(ctx) || !info || level < 0 || level >= (int)ENG(ctx, linfo.size())) return refuse(ctx);
    if (ctx->e32) fill_level(*ctx->e32, level, info); else fill_level(*ctx->e64, level, info);
    return GRLBWT_OK;
}
int grlbwt_build(grlbwt_ctx *ctx) {
    return stage(ctx, nullptr, [&] { ENG(ctx, run_all()); });
}

int grlbwt_result_size(const grlbwt_ctx *ctx, uint64_t *image_bytes, uint64_t *n_runs) {
    if (const char *why = need_image(ctx)) return refuse(ctx, why);
    if (image_bytes) *image_bytes = ENG(ctx, image_bytes);
    if (n_runs) *n_runs = ENG(ctx, image_runs);
    return GRLBWT_OK;
}
int grlbwt_result_device_ptr(const grlbwt_ctx *ctx, const void **dev_ptr) {
    if (const char *why = need_image(ctx)) return refuse(ctx, why);
    if (!dev_ptr) return refuse(ctx, "null argument");
    *dev_ptr = ENG(ctx, image.p);
    return GRLBWT_OK;
}
int grlbwt_result_download(const grlbwt_ctx *ctx, void *host_out, uint64_t capacity) {
    if (const char *why = need_image(ctx)) return refuse(ctx, why);
    if (!host_out || capacity < ENG(ctx, image_part_bytes)) return refuse(ctx, "no output buffer, or one smaller than the image");
    return guarded(const_cast<grlbwt_ctx *>(ctx), [&] { if (ENG(ctx, image_part_bytes)) prim::d2h(host_out, ENG(ctx, image.p), ENG(ctx, image_part_bytes)); });
}
int grlbwt_result_write_file(const grlbwt_ctx *ctx, const char *path) {
    if (const char *why = need_image(ctx)) return refuse(ctx, why);
    if (!path) return refuse(ctx, "null argument");
    if (ENG(ctx, image_part_bytes) != ENG(ctx, image_bytes)) return refuse(ctx, "this context holds a part of the image: grlbwt_result_write_part");
    return guarded(const_cast<grlbwt_ctx *>(ctx), [&] { write_image(ENG(ctx, image.p), ENG(ctx, image_bytes), path); });
}
int grlbwt_result_part(const grlbwt_ctx *ctx, uint64_t *offset, uint64_t *bytes) {
    if (const char *why = need_image(ctx)) return refuse(ctx, why);
    if (offset) *offset = ENG(ctx, image_part_off);
    if (bytes) *bytes = ENG(ctx, image_part_bytes);
    return GRLBWT_OK;
}
int grlbwt_result_write_part(const grlbwt_ctx *ctx, const char *path) {
    if (const char *why = need_image(ctx)) return refuse(ctx, why);
    if (!path) return refuse(ctx, "null argument");
    return guarded(const_cast<grlbwt_ctx *>(ctx), [&] { write_image(ENG(ctx, image.p), ENG(ctx, image_part_bytes), path, true, ENG(ctx, image_part_off), ENG(ctx, image_bytes)); });
}

int grlbwt_level_text_size(const grlbwt_ctx *ctx, int level, uint64_t *n_cells) {
    if (!HAS_ENG(ctx) || !n_cells || level < 1 || level > (int)ENG(ctx, kept_texts.size())) return refuse(ctx);
    *n_cells = ENG(ctx, kept_texts[level - 1].n);
    return GRLBWT_OK;
}
int grlbwt_level_text_download(const grlbwt_ctx *ctx, int level, uint64_t *cells_out) {
    if (!HAS_ENG(ctx) || !cells_out || level < 1 || level > (int)ENG(ctx, kept_texts.size())) return refuse(ctx);
    return guarded(const_cast<grlbwt_ctx *>(ctx), [&] {
        if (ctx->e32) text_download(*ctx->e32, level, cells_out); else text_download(*ctx->e64, level, cells_out);
    });
}
int grlbwt_level_bwt_size(const grlbwt_ctx *ctx, int level, uint64_t *n_runs) {
    if (!HAS_ENG(ctx) || !n_runs || level < 0 || level >= (int)ENG(ctx, kept_bwts.size())) return refuse(ctx);
    *n_runs = ENG(ctx, kept_bwts[level].R);
    return GRLBWT_OK;
}
int grlbwt_level_bwt_download(const grlbwt_ctx *ctx, int level, uint64_t *sym_out, uint64_t *len_out) {
    if (!HAS_ENG(ctx) || !sym_out || !len_out || level < 0 || level >= (int)ENG(ctx, kept_bwts.size())) return refuse(ctx);
    return guarded(const_cast<grlbwt_ctx *>(ctx), [&] {
        if (ctx->e32) bwt_download(*ctx->e32, level, sym_out, len_out); else bwt_download(*ctx->e64, level, sym_out, len_out);
    });
}

int grlbwt_level_grammar_size(const grlbwt_ctx *ctx, int level, uint64_t *n_metasyms, uint64_t *prebwt_runs) {
    if (!HAS_ENG(ctx) || level < 0 || level >= (int)ENG(ctx, levels.size())) return refuse(ctx);
    if (ENG(ctx, levels[level].g0.p) == nullptr) return GRLBWT_EINVAL;           // already consumed by the induction of this level
    if (n_metasyms) *n_metasyms = ENG(ctx, levels[level].M);
    if (prebwt_runs) *prebwt_runs = ENG(ctx, levels[level].prebwt.R);
    return GRLBWT_OK;
}
int grlbwt_level_grammar_download(const grlbwt_ctx *ctx, int level, uint64_t *g0, uint64_t *g1, uint8_t *has_hocc,
                                  uint64_t *prebwt_sym, uint64_t *prebwt_len) {
    if (grlbwt_level_grammar_size(ctx, level, nullptr, nullptr) != GRLBWT_OK) return refuse(ctx);
    return guarded(const_cast<grlbwt_ctx *>(ctx), [&] {
        if (ctx->e32) grammar_download(*ctx->e32, level, g0, g1, has_hocc, prebwt_sym, prebwt_len);
        else grammar_download(*ctx->e64, level, g0, g1, has_hocc, prebwt_sym, prebwt_len);
    });
}

int grlbwt_get_counters(const grlbwt_ctx *ctx, grlbwt_counters *out) {
    if (!HAS_ENG(ctx) || !out) return refuse(ctx);
    try { prim::sync(); } catch (...) { return GRLBWT_EDEVICE; }   // folds the stage clocks still in flight
    if (ctx->e32) fill_counters(*ctx->e32, out); else fill_counters(*ctx->e64, out);
    return GRLBWT_OK;
}

int grlbwt_invert_image_tails(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes, uint64_t tail_cells,
                              void *dev_out, uint64_t capacity_cells, uint64_t *n_strings_out, uint64_t *n_cells_out) {
    if (!ctx || !dev_image || !dev_out || tail_cells == 0) return refuse(ctx);
    return guarded(ctx, [&] {
        const uint64_t total = grl64::Image::image_total_symbols(dev_image, image_bytes);
        const bool big = idx64_for(ctx, total);
        uint64_t k = 0;
        const uint64_t n = big ? grl64::Image::invert_image_tails(dev_image, image_bytes, cell_bytes, tail_cells, dev_out, capacity_cells, &k)
                               : grl32::Image::invert_image_tails(dev_image, image_bytes, cell_bytes, tail_cells, dev_out, capacity_cells, &k);
        if (n_strings_out) *n_strings_out = k;
        if (n_cells_out) *n_cells_out = n;
    });
}

int grlbwt_invert_image(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes,
                        void *dev_text_out, uint64_t capacity_cells, uint64_t *n_cells_out) {
    if (!ctx || !dev_image || !dev_text_out) return refuse(ctx);
    return guarded(ctx, [&] {
        // the index width follows the number of symbols the image DESCRIBES (summed in 64 bits), not the buffer sizes:
        // a small image can describe >= 2^32 symbols, and a 32-bit scan of its run lengths would wrap
        const uint64_t total = grl64::Image::image_total_symbols(dev_image, image_bytes);
        if (total > capacity_cells) throw prim::Error(GRLBWT_EINVAL, "inversion: output buffer too small");
        bool big = idx64_for(ctx, total);
        uint64_t n = big ? grl64::Image::invert_image(dev_image, image_bytes, cell_bytes, dev_text_out, capacity_cells, total)
                         : grl32::Image::invert_image(dev_image, image_bytes, cell_bytes, dev_text_out, capacity_cells, total);
        if (n_cells_out) *n_cells_out = n;
    });
}


int grlbwt_fm_create(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, uint32_t fm_flags, grlbwt_fm **out) {
    if (!ctx || !dev_image || !out) return refuse(ctx);
    *out = nullptr;
    const uint32_t sample_bits = (fm_flags >> 8) & 0xFFu;
    if ((fm_flags & ~(GRLBWT_FM_LOCATE | GRLBWT_FM_CHECKPOINTS | GRLBWT_FM_EXTRACT | 0xFF00u)) || sample_bits > 20 ||
        (!(fm_flags & GRLBWT_FM_CHECKPOINTS) && sample_bits) || ((fm_flags & (GRLBWT_FM_CHECKPOINTS | GRLBWT_FM_EXTRACT)) && !(fm_flags & GRLBWT_FM_LOCATE))) {
        ctx->err = "fm index: bad flags (checkpoints and extracting need the locate structures; sample_bits is 0 or 1 to 20 and needs checkpoints)";
        return GRLBWT_EINVAL;
    }
    return guarded(ctx, [&] {
        const uint64_t total = grl64::Image::image_total_symbols(dev_image, image_bytes);
        const bool big = idx64_for(ctx, total);
        const bool locate = fm_flags & GRLBWT_FM_LOCATE, cps = fm_flags & GRLBWT_FM_CHECKPOINTS, ext = fm_flags & GRLBWT_FM_EXTRACT;
        std::unique_ptr<grlbwt_fm> fm(new grlbwt_fm());
        fm->flags = fm_flags;
        if (big) {
            fm->f64.reset(new grl64::Image::FmIndex());
            grl64::Image::fm_create(dev_image, image_bytes, locate, prim::sw().fm_top_bits, *fm->f64, cps, (int)sample_bits, ext);
        } else {
            fm->f32.reset(new grl32::Image::FmIndex());
            grl32::Image::fm_create(dev_image, image_bytes, locate, prim::sw().fm_top_bits, *fm->f32, cps, (int)sample_bits, ext);
        }
        ctx->fms.push_back(fm.get());
        *out = fm.release();
    });
}
int grlbwt_fm_destroy(grlbwt_ctx *ctx, grlbwt_fm *fm) {
    if (!ctx) return GRLBWT_EINVAL;
    if (!fm) return GRLBWT_OK;
    auto it = std::find(ctx->fms.begin(), ctx->fms.end(), fm);
    if (it == ctx->fms.end()) { ctx->err = "fm destroy: not an index of this context"; return GRLBWT_EINVAL; }
    ctx->fms.erase(it);
    return guarded(ctx, [&] { prim::sync(); delete fm; });
}
int grlbwt_fm_info_get(const grlbwt_fm *fm, grlbwt_fm_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F, uint64_t idx_bytes) {
        out->n_syms = F.n; out->n_runs = F.R; out->n_strings = F.k; out->sigma = F.sigma; out->separator = F.sepval;
        out->idx_bytes = idx_bytes; out->index_bytes = F.bytes(); out->top_entries = F.top_entries; out->flags = fm->flags;
    };
    if (fm->f32) fill(*fm->f32, 4); else fill(*fm->f64, 8);
    return GRLBWT_OK;
}
static const auto fill_walk_info = [](const auto &w, grlbwt_walk_info *out) {
    out->n_strings = w.k; out->n_checkpoints = w.m; out->sample_bits = w.b;
    out->longest_segment = w.longest_segment; out->longest_chain = w.longest_chain; out->jump_rounds = w.jump_rounds;
    out->walk_lanes = w.lanes; out->lane_refills = w.refills; out->scratch_bytes = w.scratch_bytes; out->sample_bytes = w.sample_bytes;
};
int grlbwt_fm_walk_info_get(const grlbwt_fm *fm, grlbwt_walk_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    if (fm->f32 ? !fm->f32->checkpoints : !fm->f64->checkpoints) return GRLBWT_EINVAL;
    if (fm->f32) fill_walk_info(fm->f32->walk, out); else fill_walk_info(fm->f64->walk, out);
    return GRLBWT_OK;
}
int grlbwt_invert_image_checkpointed(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes, int sample_bits,
                                     void *dev_text_out, uint64_t capacity_cells, uint64_t *n_cells_out, grlbwt_walk_info *info) {
    if (!ctx || !dev_image || !dev_text_out) return refuse(ctx);
    return guarded(ctx, [&] {
        if (sample_bits < 0 || sample_bits > 20) throw prim::Error(GRLBWT_EINVAL, "checkpointed walk: sample_bits is 0 (the default) or 1 to 20");
        const uint64_t total = grl64::Image::image_total_symbols(dev_image, image_bytes);
        if (total > capacity_cells) throw prim::Error(GRLBWT_EINVAL, "inversion: output buffer too small");
        const bool big = idx64_for(ctx, total);
        uint64_t n;
        grlbwt_walk_info wi;
        if (big) {
            grl64::Image::WalkInfo w;
            n = grl64::Image::invert_image_checkpointed(dev_image, image_bytes, cell_bytes, sample_bits, dev_text_out, capacity_cells, w);
            fill_walk_info(w, &wi);
        } else {
            grl32::Image::WalkInfo w;
            n = grl32::Image::invert_image_checkpointed(dev_image, image_bytes, cell_bytes, sample_bits, dev_text_out, capacity_cells, w);
            fill_walk_info(w, &wi);
        }
        if (n_cells_out) *n_cells_out = n;
        if (info) *info = wi;
    });
}
int grlbwt_fm_count(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                    uint64_t n_patterns, uint64_t *dev_lo, uint64_t *dev_hi) {
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_patterns && (!dev_offsets || !dev_lo || !dev_hi)) return GRLBWT_EINVAL;
    return guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_count(*fm->f32, dev_cells, cell_bytes, dev_offsets, n_patterns, dev_lo, dev_hi);
        else grl64::Image::fm_count(*fm->f64, dev_cells, cell_bytes, dev_offsets, n_patterns, dev_lo, dev_hi);
    });
}
int grlbwt_fm_match(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                    uint64_t n_patterns, uint64_t max_len, uint64_t *dev_len, uint64_t *dev_lo, uint64_t *dev_hi) {
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_patterns && !dev_offsets) return GRLBWT_EINVAL;
    return guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_match(*fm->f32, dev_cells, cell_bytes, dev_offsets, n_patterns, max_len, dev_len, dev_lo, dev_hi);
        else grl64::Image::fm_match(*fm->f64, dev_cells, cell_bytes, dev_offsets, n_patterns, max_len, dev_len, dev_lo, dev_hi);
    });
}
int grlbwt_fm_mems(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                   uint64_t n_patterns, uint64_t min_len, uint64_t max_len, uint64_t *dev_pattern, uint64_t *dev_begin, uint64_t *dev_mlen,
                   uint64_t *dev_lo, uint64_t *dev_hi, uint64_t capacity, uint64_t *n_mems_out) {
    if (n_mems_out) *n_mems_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_patterns && !dev_offsets) return GRLBWT_EINVAL;
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_mems(*fm->f32, dev_cells, cell_bytes, dev_offsets, n_patterns, min_len, max_len, dev_pattern, dev_begin, dev_mlen,
                                            dev_lo, dev_hi, capacity, n);
        else grl64::Image::fm_mems(*fm->f64, dev_cells, cell_bytes, dev_offsets, n_patterns, min_len, max_len, dev_pattern, dev_begin, dev_mlen,
                                    dev_lo, dev_hi, capacity, n);
    });
    if (n_mems_out) *n_mems_out = n;
    return rc;
}
int grlbwt_fm_match_info_get(const grlbwt_fm *fm, grlbwt_fm_match_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &m = F.minfo;
        out->n_patterns = m.patterns; out->n_cells = m.cells; out->matched_cells = m.matched; out->longest = m.longest;
        out->n_capped = m.capped; out->n_mems = m.mems; out->walk_lanes = m.lanes; out->lane_refills = m.refills;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_approx(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                     uint64_t n_patterns, uint32_t max_mismatches, uint64_t max_hits, uint64_t *dev_hit_offsets, uint64_t *dev_mism,
                     uint64_t *dev_lo, uint64_t *dev_hi, uint64_t *dev_sub_pos, uint64_t *dev_sub_val, uint64_t capacity, uint64_t *n_hits_out) {
    if (n_hits_out) *n_hits_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_patterns && !dev_offsets) return GRLBWT_EINVAL;
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_approx(*fm->f32, dev_cells, cell_bytes, dev_offsets, n_patterns, max_mismatches, max_hits, dev_hit_offsets, dev_mism,
                                              dev_lo, dev_hi, dev_sub_pos, dev_sub_val, capacity, n);
        else grl64::Image::fm_approx(*fm->f64, dev_cells, cell_bytes, dev_offsets, n_patterns, max_mismatches, max_hits, dev_hit_offsets, dev_mism,
                                      dev_lo, dev_hi, dev_sub_pos, dev_sub_val, capacity, n);
    });
    if (n_hits_out) *n_hits_out = n;
    return rc;
}
int grlbwt_fm_approx_info_get(const grlbwt_fm *fm, grlbwt_fm_approx_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &a = F.ainfo;
        out->n_patterns = a.patterns; out->n_cells = a.cells; out->max_mismatches = a.k; out->max_hits = a.max_hits;
        out->n_hits = a.hits;
        for (int d = 0; d < 4; d++) out->hits_by_mismatches[d] = a.by[d];
        out->n_truncated = a.cut; out->steps = a.steps; out->walk_lanes = a.lanes; out->lane_refills = a.refills;
        out->table_bytes = 0;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_overlaps(grlbwt_ctx *ctx, const grlbwt_fm *fm, const void *dev_cells, int cell_bytes, const uint64_t *dev_offsets,
                       uint64_t n_patterns, uint64_t min_len, uint64_t max_len, uint32_t flags, uint64_t *dev_hit_offsets, uint64_t *dev_len,
                       uint64_t *dev_tlo, uint64_t *dev_thi, uint64_t *dev_lo, uint64_t *dev_hi, uint64_t capacity, uint64_t *n_hits_out) {
    if (n_hits_out) *n_hits_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_patterns && !dev_offsets) return GRLBWT_EINVAL;
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_overlaps(*fm->f32, dev_cells, cell_bytes, dev_offsets, n_patterns, min_len, max_len, flags, dev_hit_offsets, dev_len,
                                                dev_tlo, dev_thi, dev_lo, dev_hi, capacity, n);
        else grl64::Image::fm_overlaps(*fm->f64, dev_cells, cell_bytes, dev_offsets, n_patterns, min_len, max_len, flags, dev_hit_offsets, dev_len,
                                        dev_tlo, dev_thi, dev_lo, dev_hi, capacity, n);
    });
    if (n_hits_out) *n_hits_out = n;
    return rc;
}
int grlbwt_fm_overlaps_of(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_ids, uint64_t n_ids, uint64_t min_len, uint64_t max_len,
                          uint32_t flags, uint64_t *dev_hit_offsets, uint64_t *dev_len, uint64_t *dev_tlo, uint64_t *dev_thi, uint64_t *dev_lo,
                          uint64_t *dev_hi, uint64_t capacity, uint64_t *n_hits_out) {
    if (n_hits_out) *n_hits_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_ids && !dev_ids) return GRLBWT_EINVAL;
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_overlaps_of(*fm->f32, dev_ids, n_ids, min_len, max_len, flags, dev_hit_offsets, dev_len, dev_tlo, dev_thi, dev_lo, dev_hi,
                                                   capacity, n);
        else grl64::Image::fm_overlaps_of(*fm->f64, dev_ids, n_ids, min_len, max_len, flags, dev_hit_offsets, dev_len, dev_tlo, dev_thi, dev_lo, dev_hi,
                                           capacity, n);
    });
    if (n_hits_out) *n_hits_out = n;
    return rc;
}
int grlbwt_fm_overlap_targets(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_tlo, const uint64_t *dev_thi, uint64_t n_ranges,
                              uint64_t *dev_entry_offsets, uint64_t *dev_string, uint64_t *dev_range, uint64_t capacity, uint64_t *n_entries_out) {
    if (n_entries_out) *n_entries_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_ranges && (!dev_tlo || !dev_thi)) return GRLBWT_EINVAL;
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_overlap_targets(*fm->f32, dev_tlo, dev_thi, n_ranges, dev_entry_offsets, dev_string, dev_range, capacity, n);
        else grl64::Image::fm_overlap_targets(*fm->f64, dev_tlo, dev_thi, n_ranges, dev_entry_offsets, dev_string, dev_range, capacity, n);
    });
    if (n_entries_out) *n_entries_out = n;
    return rc;
}
int grlbwt_fm_overlap_info_get(const grlbwt_fm *fm, grlbwt_fm_overlap_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &o = F.oinfo;
        out->n_patterns = o.patterns; out->n_cells = o.cells; out->n_hits = o.hits; out->n_targets = o.targets; out->longest = o.longest;
        out->steps = o.steps; out->walk_lanes = o.lanes; out->lane_refills = o.refills; out->n_ranges = o.ranges; out->n_entries = o.entries;
        out->tile_entries = o.tile;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_lcp(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t max_lcp, int lcp_bytes, void *dev_lcp, uint64_t *host_rows_at,
                  uint64_t *host_suffixes_of, uint64_t hist_capacity, uint64_t *n_levels_out) {
    if (n_levels_out) *n_levels_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_lcp(*fm->f32, max_lcp, lcp_bytes, dev_lcp, host_rows_at, host_suffixes_of, hist_capacity, n);
        else grl64::Image::fm_lcp(*fm->f64, max_lcp, lcp_bytes, dev_lcp, host_rows_at, host_suffixes_of, hist_capacity, n);
    });
    if (n_levels_out) *n_levels_out = n;
    return rc;
}
int grlbwt_fm_lcp_info_get(const grlbwt_fm *fm, grlbwt_fm_lcp_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &l = F.linfo;
        out->n_rows = l.n; out->n_strings = l.k; out->lcp_bytes = l.lcp_bytes; out->cap = l.cap;
        out->passes = l.passes; out->n_levels = l.n_levels; out->max_lcp = l.max_lcp; out->n_capped = l.n_capped;
        out->tile_rows = l.tile_rows; out->scratch_bytes = l.scratch_bytes;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_sa(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t row_begin, uint64_t row_end, int string_bytes, void *dev_string, int offset_bytes,
                 void *dev_offset) {
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_sa(*fm->f32, row_begin, row_end, string_bytes, dev_string, offset_bytes, dev_offset);
        else grl64::Image::fm_sa(*fm->f64, row_begin, row_end, string_bytes, dev_string, offset_bytes, dev_offset);
    });
}
int grlbwt_fm_sa_info_get(const grlbwt_fm *fm, grlbwt_fm_sa_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &s = F.sinfo;
        out->n_rows = s.n; out->n_strings = s.k; out->row_begin = s.row_begin; out->row_end = s.row_end;
        out->string_bytes = s.string_bytes; out->offset_bytes = s.offset_bytes; out->n_written = s.written; out->form = s.form;
        out->walk_steps = s.steps; out->longest_walk = s.longest; out->walk_lanes = s.lanes; out->lane_refills = s.refills;
        out->scratch_bytes = s.scratch_bytes;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_kmers(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count, uint64_t row_begin, uint64_t row_end,
                    int cell_bytes, void *dev_cells, uint64_t *dev_lo, uint64_t *dev_count, uint64_t capacity, uint64_t *n_kmers_out,
                    uint64_t *host_spectrum, uint64_t spectrum_bins) {
    if (n_kmers_out) *n_kmers_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_kmers(*fm->f32, k, min_count, max_count, row_begin, row_end, cell_bytes, dev_cells, dev_lo, dev_count, capacity, n,
                                            n_kmers_out != nullptr, host_spectrum, spectrum_bins);
        else grl64::Image::fm_kmers(*fm->f64, k, min_count, max_count, row_begin, row_end, cell_bytes, dev_cells, dev_lo, dev_count, capacity, n,
                                    n_kmers_out != nullptr, host_spectrum, spectrum_bins);
    });
    if (n_kmers_out) *n_kmers_out = n;
    return rc;
}
int grlbwt_fm_kmer_info_get(const grlbwt_fm *fm, grlbwt_fm_kmer_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &i = F.kinfo;
        out->k = i.k; out->n_rows = i.n; out->n_strings = i.n_strings; out->n_distinct = i.n_distinct; out->n_windows = i.n_windows;
        out->n_selected = i.n_selected; out->largest_count = i.largest_count; out->passes = i.passes; out->length_passes = i.length_passes;
        out->forward_steps = i.forward_steps; out->tile_rows = i.tile_rows; out->tile_kmers = i.tile_kmers; out->stage_bytes = i.stage_bytes;
        out->scratch_bytes = i.scratch_bytes;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_kmers_canonical(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count, uint64_t row_begin, uint64_t row_end,
                              const uint64_t *host_pairs, uint64_t n_pairs, int cell_bytes, void *dev_cells, uint64_t *dev_lo, uint64_t *dev_count,
                              uint64_t *dev_mate_lo, uint64_t *dev_total, uint64_t capacity, uint64_t *n_classes_out, uint64_t *host_spectrum,
                              uint64_t spectrum_bins) {
    if (n_classes_out) *n_classes_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_ckmers(*fm->f32, k, min_count, max_count, row_begin, row_end, host_pairs, n_pairs, cell_bytes, dev_cells, dev_lo, dev_count,
                                             dev_mate_lo, dev_total, capacity, n, n_classes_out != nullptr, host_spectrum, spectrum_bins);
        else grl64::Image::fm_ckmers(*fm->f64, k, min_count, max_count, row_begin, row_end, host_pairs, n_pairs, cell_bytes, dev_cells, dev_lo, dev_count,
                                     dev_mate_lo, dev_total, capacity, n, n_classes_out != nullptr, host_spectrum, spectrum_bins);
    });
    if (n_classes_out) *n_classes_out = n;
    return rc;
}
int grlbwt_fm_kmers_canonical_info_get(const grlbwt_fm *fm, grlbwt_fm_ckmer_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &i = F.cinfo;
        out->k = i.k; out->n_rows = i.n; out->n_strings = i.n_strings; out->n_distinct = i.n_distinct; out->n_windows = i.n_windows;
        out->n_selected = i.n_selected; out->n_classes = i.n_classes; out->n_paired = i.n_paired; out->n_palindromes = i.n_palindromes;
        out->n_single = i.n_single; out->n_no_complement = i.n_no_complement; out->largest_total = i.largest_total; out->passes = i.passes;
        out->length_passes = i.length_passes; out->mate_walks = i.mate_walks; out->backward_steps = i.backward_steps;
        out->forward_steps = i.forward_steps; out->tile_rows = i.tile_rows; out->tile_kmers = i.tile_kmers; out->mate_tile = i.mate_tile;
        out->stage_bytes = i.stage_bytes; out->scratch_bytes = i.scratch_bytes;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_repeats(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t min_len, uint64_t max_len, uint64_t min_count, uint64_t max_count, uint32_t repeat_flags,
                      uint64_t row_begin, uint64_t row_end, uint64_t *dev_lo, uint64_t *dev_count, uint64_t *dev_len, uint64_t *dev_split, uint64_t capacity,
                      uint64_t *n_repeats_out) {
    if (n_repeats_out) *n_repeats_out = 0;
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_repeats(*fm->f32, min_len, max_len, min_count, max_count, repeat_flags, row_begin, row_end, dev_lo, dev_count, dev_len,
                                              dev_split, capacity, n, n_repeats_out != nullptr);
        else grl64::Image::fm_repeats(*fm->f64, min_len, max_len, min_count, max_count, repeat_flags, row_begin, row_end, dev_lo, dev_count, dev_len,
                                      dev_split, capacity, n, n_repeats_out != nullptr);
    });
    if (n_repeats_out) *n_repeats_out = n;
    return rc;
}
int grlbwt_fm_repeat_info_get(const grlbwt_fm *fm, grlbwt_fm_repeat_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &i = F.rinfo;
        out->n_rows = i.n; out->n_strings = i.n_strings; out->min_len = i.min_len; out->max_len = i.max_len; out->passes = i.passes;
        out->n_repeats = i.n_repeats; out->n_maximal = i.n_maximal; out->n_selected = i.n_selected; out->longest = i.longest;
        out->largest_count = i.largest_count; out->value_bytes = i.value_bytes; out->tile_rows = i.tile_rows; out->tree_fanout = i.tree_fanout;
        out->tree_levels = i.tree_levels; out->far_searches = i.far_searches; out->scratch_bytes = i.scratch_bytes;
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}
int grlbwt_fm_locate(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_rows, uint64_t n_rows, uint64_t max_steps,
                     uint64_t *dev_string, uint64_t *dev_offset) {
    if (!ctx || !fm || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_rows && (!dev_rows || !dev_string || !dev_offset)) return GRLBWT_EINVAL;
    return guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_locate(*fm->f32, dev_rows, n_rows, max_steps, dev_string, dev_offset);
        else grl64::Image::fm_locate(*fm->f64, dev_rows, n_rows, max_steps, dev_string, dev_offset);
    });
}
int grlbwt_fm_string_lengths(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t *dev_len) {
    if (!ctx || !fm || !dev_len || !(fm->f32 || fm->f64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (fm->f32) grl32::Image::fm_string_lengths(*fm->f32, dev_len);
        else grl64::Image::fm_string_lengths(*fm->f64, dev_len);
    });
}
int grlbwt_fm_extract(grlbwt_ctx *ctx, const grlbwt_fm *fm, const uint64_t *dev_string, const uint64_t *dev_begin, const uint64_t *dev_end,
                      uint64_t n_ranges, int cell_bytes, void *dev_out, uint64_t capacity_cells, uint64_t *dev_out_offsets, uint64_t *n_cells_out) {
    if (!ctx || !fm || !dev_out_offsets || !(fm->f32 || fm->f64)) return refuse(ctx);
    if (n_ranges && (!dev_string || !dev_begin || !dev_end || (!dev_out && capacity_cells))) return GRLBWT_EINVAL;
    return guarded(ctx, [&] {
        const uint64_t n = fm->f32 ? grl32::Image::fm_extract(*fm->f32, dev_string, dev_begin, dev_end, n_ranges, cell_bytes, dev_out, capacity_cells, dev_out_offsets)
                                   : grl64::Image::fm_extract(*fm->f64, dev_string, dev_begin, dev_end, n_ranges, cell_bytes, dev_out, capacity_cells, dev_out_offsets);
        if (n_cells_out) *n_cells_out = n;
    });
}
int grlbwt_fm_extract_info_get(const grlbwt_fm *fm, grlbwt_fm_extract_info *out) {
    if (!fm || !out || !(fm->f32 || fm->f64)) return GRLBWT_EINVAL;
    if (fm->f32 ? !fm->f32->extract : !fm->f64->extract) return GRLBWT_EINVAL;
    auto fill = [&](const auto &F) {
        const auto &x = F.xinfo;
        out->n_ranges = x.ranges; out->n_pieces = x.pieces; out->n_cells = x.cells; out->walk_steps = x.steps;
        out->walk_lanes = x.lanes; out->lane_refills = x.refills; out->n_samples = F.xq.n; out->extract_bytes = F.extract_bytes();
    };
    if (fm->f32) fill(*fm->f32); else fill(*fm->f64);
    return GRLBWT_OK;
}

int grlbwt_merge_create(grlbwt_ctx *ctx, const void *dev_image_a, uint64_t bytes_a, const void *dev_image_b, uint64_t bytes_b, int cell_bytes,
                        uint64_t max_rounds, grlbwt_merge **out) {
    if (out) *out = nullptr;
    if (!ctx || !dev_image_a || !dev_image_b || !out) return refuse(ctx);
    return guarded(ctx, [&] {
        const uint64_t ta = grl64::Image::image_total_symbols(dev_image_a, bytes_a), tb = grl64::Image::image_total_symbols(dev_image_b, bytes_b);
        if (ta >= kMergeRowLimit || tb >= kMergeRowLimit || ta + tb >= kMergeRowLimit) throw prim::Error(GRLBWT_ERANGE, "merge: 2^40 merged rows or more");
        const bool big = idx64_for(ctx, ta + tb);
        std::unique_ptr<grlbwt_merge> mg(new grlbwt_merge());
        if (big) {
            mg->m64.reset(new grl64::Image::ImageMerge());
            grl64::Image::merge_create(dev_image_a, bytes_a, dev_image_b, bytes_b, cell_bytes, max_rounds, *mg->m64);
        } else {
            mg->m32.reset(new grl32::Image::ImageMerge());
            grl32::Image::merge_create(dev_image_a, bytes_a, dev_image_b, bytes_b, cell_bytes, max_rounds, *mg->m32);
        }
        ctx->merges.push_back(mg.get());
        *out = mg.release();
    });
}
int grlbwt_merge_destroy(grlbwt_ctx *ctx, grlbwt_merge *mg) {
    if (!ctx) return GRLBWT_EINVAL;
    if (!mg) return GRLBWT_OK;
    auto it = std::find(ctx->merges.begin(), ctx->merges.end(), mg);
    if (it == ctx->merges.end()) { ctx->err = "merge destroy: not a merge of this context"; return GRLBWT_EINVAL; }
    ctx->merges.erase(it);
    return guarded(ctx, [&] { prim::sync(); delete mg; });
}
int grlbwt_merge_info_get(const grlbwt_merge *mg, grlbwt_merge_info *out) {
    if (!mg || !out || !(mg->m32 || mg->m64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &M, uint64_t idx_bytes, uint64_t tile_rows) {
        out->n_syms_a = M.na; out->n_syms_b = M.nb; out->n_strings_a = M.ka; out->n_strings_b = M.kb;
        out->sigma = M.sigma; out->separator = M.sepval; out->rounds = M.rounds; out->rows_changed = M.rows_changed;
        out->n_runs = M.n_runs; out->out_bytes = M.out_bytes; out->sb = M.sb; out->fb = M.fb;
        out->idx_bytes = idx_bytes; out->tile_rows = tile_rows; out->scratch_bytes = M.scratch_bytes; out->held_bytes = M.held_bytes();
    };
    if (mg->m32) fill(*mg->m32, 4, grl32::Image::kMergeTile); else fill(*mg->m64, 8, grl64::Image::kMergeTile);
    return GRLBWT_OK;
}
int grlbwt_merge_emit(grlbwt_ctx *ctx, const grlbwt_merge *mg, void *dev_out, uint64_t capacity_bytes) {
    if (!ctx || !mg || !dev_out || !(mg->m32 || mg->m64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (mg->m32) grl32::Image::merge_emit(*mg->m32, (uint8_t *)dev_out, capacity_bytes);
        else grl64::Image::merge_emit(*mg->m64, (uint8_t *)dev_out, capacity_bytes);
    });
}
int grlbwt_merge_interleave(grlbwt_ctx *ctx, const grlbwt_merge *mg, uint64_t *dev_bits) {
    if (!ctx || !mg || !dev_bits || !(mg->m32 || mg->m64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (mg->m32) grl32::Image::merge_interleave(*mg->m32, dev_bits);
        else grl64::Image::merge_interleave(*mg->m64, dev_bits);
    });
}
int grlbwt_merge_files(grlbwt_ctx *ctx, const char *path_a, const char *path_b, int cell_bytes, uint64_t max_rounds, const char *path_out,
                       grlbwt_merge_info *info) {
    if (!ctx || !path_a || !path_b || !path_out) return refuse(ctx);
    grlbwt_merge *mg = nullptr;
    int rc = guarded(ctx, [&] {
        RawText a, b;
        read_image_file(path_a, a);
        read_image_file(path_b, b);
        const int r = grlbwt_merge_create(ctx, a.buf.p, a.n, b.buf.p, b.n, cell_bytes, max_rounds, &mg);
        if (r != GRLBWT_OK) throw prim::Error(r, ctx->err);
    });
    if (rc != GRLBWT_OK) return rc;
    rc = guarded(ctx, [&] {
        grlbwt_merge_info mi;
        grlbwt_merge_info_get(mg, &mi);
        grl64::DBuf<uint8_t> out(mi.out_bytes);
        const int r = grlbwt_merge_emit(ctx, mg, out.p, mi.out_bytes);
        if (r != GRLBWT_OK) throw prim::Error(r, ctx->err);
        write_image(out.p, mi.out_bytes, path_out);
        if (info) *info = mi;
    });
    const std::string err = ctx->err;
    grlbwt_merge_destroy(ctx, mg);
    if (rc != GRLBWT_OK) ctx->err = err;
    return rc;
}

int grlbwt_docs_create(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint32_t docs_flags, grlbwt_docs **out) {
    if (out) *out = nullptr;
    if (!ctx || !fm || !out || !(fm->f32 || fm->f64)) return refuse(ctx);
    return guarded(ctx, [&] {
        std::unique_ptr<grlbwt_docs> dc(new grlbwt_docs());
        if (fm->f32) {
            dc->d32.reset(new grl32::Image::ImageDocs());
            grl32::Image::docs_create(*fm->f32, docs_flags, *dc->d32);
        } else {
            dc->d64.reset(new grl64::Image::ImageDocs());
            grl64::Image::docs_create(*fm->f64, docs_flags, *dc->d64);
        }
        ctx->docs.push_back(dc.get());
        *out = dc.release();
    });
}
int grlbwt_docs_destroy(grlbwt_ctx *ctx, grlbwt_docs *dc) {
    if (!ctx) return GRLBWT_EINVAL;
    if (!dc) return GRLBWT_OK;
    auto it = std::find(ctx->docs.begin(), ctx->docs.end(), dc);
    if (it == ctx->docs.end()) { ctx->err = "docs destroy: not a handle of this context"; return GRLBWT_EINVAL; }
    ctx->docs.erase(it);
    return guarded(ctx, [&] { prim::sync(); delete dc; });
}
int grlbwt_docs_info_get(const grlbwt_docs *dc, grlbwt_docs_info *out) {
    if (!dc || !out || !(dc->d32 || dc->d64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &D, uint64_t idx_bytes, uint64_t tile) {
        out->n_rows = D.n; out->n_strings = D.k; out->flags = D.flags; out->idx_bytes = idx_bytes; out->held_bytes = D.held_bytes();
        out->scratch_bytes = D.scratch_bytes; out->sort_bits = D.sort_bits; out->form = D.form; out->walk_steps = D.steps;
        out->n_ranges = D.q.ranges; out->n_range_rows = D.q.range_rows; out->n_entries = D.q.entries; out->largest_range = D.q.largest;
        out->most_docs = D.q.most; out->tile_entries = tile;
    };
    if (dc->d32) fill(*dc->d32, 4, grl32::Image::kDocsTile); else fill(*dc->d64, 8, grl64::Image::kDocsTile);
    return GRLBWT_OK;
}
int grlbwt_docs_count(grlbwt_ctx *ctx, const grlbwt_docs *dc, const uint64_t *dev_lo, const uint64_t *dev_hi, uint64_t n_ranges, uint64_t *dev_ndocs,
                      uint64_t *n_docs_total_out) {
    if (n_docs_total_out) *n_docs_total_out = 0;
    if (!ctx || !dc || !(dc->d32 || dc->d64)) return refuse(ctx);
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (dc->d32) grl32::Image::docs_query(*dc->d32, dev_lo, dev_hi, n_ranges, false, dev_ndocs, nullptr, nullptr, nullptr, nullptr, nullptr, 0, n);
        else grl64::Image::docs_query(*dc->d64, dev_lo, dev_hi, n_ranges, false, dev_ndocs, nullptr, nullptr, nullptr, nullptr, nullptr, 0, n);
    });
    if (n_docs_total_out) *n_docs_total_out = n;
    return rc;
}
int grlbwt_docs_list(grlbwt_ctx *ctx, const grlbwt_docs *dc, const uint64_t *dev_lo, const uint64_t *dev_hi, uint64_t n_ranges, uint64_t *dev_entry_offsets,
                     uint64_t *dev_string, uint64_t *dev_first_row, uint64_t *dev_occ, uint64_t *dev_range, uint64_t capacity, uint64_t *n_entries_out) {
    if (n_entries_out) *n_entries_out = 0;
    if (!ctx || !dc || !(dc->d32 || dc->d64)) return refuse(ctx);
    uint64_t n = 0;
    const int rc = guarded(ctx, [&] {
        if (dc->d32) grl32::Image::docs_query(*dc->d32, dev_lo, dev_hi, n_ranges, true, nullptr, dev_entry_offsets, dev_string, dev_first_row, dev_occ, dev_range, capacity, n);
        else grl64::Image::docs_query(*dc->d64, dev_lo, dev_hi, n_ranges, true, nullptr, dev_entry_offsets, dev_string, dev_first_row, dev_occ, dev_range, capacity, n);
    });
    if (n_entries_out) *n_entries_out = n;
    return rc;
}

int grlbwt_debruijn_create(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count, uint32_t debruijn_flags,
                           grlbwt_debruijn **out) {
    if (out) *out = nullptr;
    if (!ctx || !fm || !out || !(fm->f32 || fm->f64)) return refuse(ctx);
    return guarded(ctx, [&] {
        std::unique_ptr<grlbwt_debruijn> g(new grlbwt_debruijn());
        if (fm->f32) {
            g->g32.reset(new grl32::Image::ImageDeBruijn());
            grl32::Image::debruijn_create(*fm->f32, k, min_count, max_count, debruijn_flags, *g->g32);
        } else {
            g->g64.reset(new grl64::Image::ImageDeBruijn());
            grl64::Image::debruijn_create(*fm->f64, k, min_count, max_count, debruijn_flags, *g->g64);
        }
        ctx->graphs.push_back(g.get());
        *out = g.release();
    });
}
int grlbwt_debruijn_destroy(grlbwt_ctx *ctx, grlbwt_debruijn *graph) {
    if (!ctx) return GRLBWT_EINVAL;
    if (!graph) return GRLBWT_OK;
    auto it = std::find(ctx->graphs.begin(), ctx->graphs.end(), graph);
    if (it == ctx->graphs.end()) { ctx->err = "de bruijn destroy: not a handle of this context"; return GRLBWT_EINVAL; }
    ctx->graphs.erase(it);
    return guarded(ctx, [&] { prim::sync(); delete graph; });
}
int grlbwt_debruijn_info_get(const grlbwt_debruijn *graph, grlbwt_debruijn_info *out) {
    if (!graph || !out || !(graph->g32 || graph->g64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &G, uint64_t tile_nodes, uint64_t tile_cells) {
        const auto &i = G.i;
        out->k = i.k; out->n_rows = i.n; out->n_strings = i.n_strings; out->n_distinct = i.n_distinct; out->n_nodes = i.n_nodes; out->n_edges = i.n_edges;
        out->n_unitigs = i.n_unitigs; out->n_circular = i.n_circular; out->longest_unitig = i.longest; out->n_cells = i.n_cells;
        out->max_in_degree = i.max_in; out->max_out_degree = i.max_out; out->passes = i.passes; out->length_passes = i.length_passes;
        out->backward_steps = i.backward_steps; out->jump_rounds = i.jump_rounds; out->tile_nodes = tile_nodes; out->tile_cells = tile_cells;
        out->handle_bytes = G.held_bytes(); out->scratch_bytes = i.scratch_bytes;
    };
    if (graph->g32) fill(*graph->g32, grl32::Image::kDbTileNodes, grl32::Image::kDbTileCells);
    else fill(*graph->g64, grl64::Image::kDbTileNodes, grl64::Image::kDbTileCells);
    return GRLBWT_OK;
}
int grlbwt_debruijn_nodes(grlbwt_ctx *ctx, const grlbwt_debruijn *graph, uint64_t *dev_lo, uint64_t *dev_count, uint32_t *dev_in_degree,
                          uint32_t *dev_out_degree, uint64_t *dev_unitig, uint64_t *dev_rank, uint64_t capacity) {
    if (!ctx || !graph || !(graph->g32 || graph->g64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (graph->g32) grl32::Image::debruijn_nodes(*graph->g32, dev_lo, dev_count, dev_in_degree, dev_out_degree, dev_unitig, dev_rank, capacity);
        else grl64::Image::debruijn_nodes(*graph->g64, dev_lo, dev_count, dev_in_degree, dev_out_degree, dev_unitig, dev_rank, capacity);
    });
}
int grlbwt_debruijn_edges(grlbwt_ctx *ctx, const grlbwt_debruijn *graph, uint64_t *dev_in_offsets, uint64_t *dev_from, uint64_t *dev_weight,
                          uint64_t *dev_row, uint64_t capacity) {
    if (!ctx || !graph || !(graph->g32 || graph->g64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (graph->g32) grl32::Image::debruijn_edges(*graph->g32, dev_in_offsets, dev_from, dev_weight, dev_row, capacity);
        else grl64::Image::debruijn_edges(*graph->g64, dev_in_offsets, dev_from, dev_weight, dev_row, capacity);
    });
}
int grlbwt_debruijn_unitigs(grlbwt_ctx *ctx, const grlbwt_debruijn *graph, const grlbwt_fm *fm, int cell_bytes, uint64_t *dev_node_offsets,
                            uint64_t *dev_nodes, void *dev_cells, uint64_t *dev_weight, uint8_t *dev_circular, uint64_t capacity_unitigs,
                            uint64_t capacity_nodes, uint64_t capacity_cells) {
    if (!ctx || !graph || !(graph->g32 || graph->g64)) return refuse(ctx);
    if (fm && (graph->g32 ? !fm->f32 : !fm->f64)) return refuse(ctx, "de bruijn unitigs: not the index the graph was made from");
    return guarded(ctx, [&] {
        if (graph->g32) grl32::Image::debruijn_unitigs(*graph->g32, fm ? fm->f32.get() : nullptr, cell_bytes, dev_node_offsets, dev_nodes, dev_cells,
                                                       dev_weight, dev_circular, capacity_unitigs, capacity_nodes, capacity_cells);
        else grl64::Image::debruijn_unitigs(*graph->g64, fm ? fm->f64.get() : nullptr, cell_bytes, dev_node_offsets, dev_nodes, dev_cells, dev_weight,
                                            dev_circular, capacity_unitigs, capacity_nodes, capacity_cells);
    });
}

int grlbwt_cdebruijn_create(grlbwt_ctx *ctx, const grlbwt_fm *fm, uint64_t k, uint64_t min_count, uint64_t max_count, const uint64_t *host_pairs,
                            uint64_t n_pairs, uint32_t cdebruijn_flags, grlbwt_cdebruijn **out) {
    if (out) *out = nullptr;
    if (!ctx || !fm || !out || !(fm->f32 || fm->f64)) return refuse(ctx);
    return guarded(ctx, [&] {
        std::unique_ptr<grlbwt_cdebruijn> g(new grlbwt_cdebruijn());
        if (fm->f32) {
            g->g32.reset(new grl32::Image::ImageCDeBruijn());
            grl32::Image::cdebruijn_create(*fm->f32, k, min_count, max_count, host_pairs, n_pairs, cdebruijn_flags, *g->g32);
        } else {
            g->g64.reset(new grl64::Image::ImageCDeBruijn());
            grl64::Image::cdebruijn_create(*fm->f64, k, min_count, max_count, host_pairs, n_pairs, cdebruijn_flags, *g->g64);
        }
        ctx->cgraphs.push_back(g.get());
        *out = g.release();
    });
}
int grlbwt_cdebruijn_destroy(grlbwt_ctx *ctx, grlbwt_cdebruijn *graph) {
    if (!ctx) return GRLBWT_EINVAL;
    if (!graph) return GRLBWT_OK;
    auto it = std::find(ctx->cgraphs.begin(), ctx->cgraphs.end(), graph);
    if (it == ctx->cgraphs.end()) { ctx->err = "canonical de bruijn destroy: not a handle of this context"; return GRLBWT_EINVAL; }
    ctx->cgraphs.erase(it);
    return guarded(ctx, [&] { prim::sync(); delete graph; });
}
int grlbwt_cdebruijn_info_get(const grlbwt_cdebruijn *graph, grlbwt_cdebruijn_info *out) {
    if (!graph || !out || !(graph->g32 || graph->g64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &G, uint64_t tile_nodes, uint64_t tile_cells) {
        const auto &i = G.i;
        out->k = i.k; out->n_rows = i.n; out->n_strings = i.n_strings; out->n_distinct = i.n_distinct; out->n_nodes = i.n_nodes; out->n_rigid = i.n_rigid;
        out->n_palindromes = i.n_palindromes; out->n_edges = i.n_edges; out->n_half_edges = i.n_half_edges; out->n_hairpins = i.n_hairpins;
        out->n_unitigs = i.n_unitigs; out->n_circular = i.n_circular; out->longest_unitig = i.longest; out->n_cells = i.n_cells;
        out->max_end_degree = i.max_end_degree; out->passes = i.passes; out->length_passes = i.length_passes;
        out->mate_backward_steps = i.mate_backward_steps; out->edge_backward_steps = i.edge_backward_steps; out->forward_steps = i.forward_steps;
        out->cells_forward_steps = G.cells_forward_steps; out->jump_rounds = i.jump_rounds; out->tile_nodes = tile_nodes; out->tile_cells = tile_cells;
        out->handle_bytes = G.held_bytes(); out->scratch_bytes = i.scratch_bytes;
    };
    if (graph->g32) fill(*graph->g32, grl32::Image::kCdbTileNodes, grl32::Image::kCdbTileCells);
    else fill(*graph->g64, grl64::Image::kCdbTileNodes, grl64::Image::kCdbTileCells);
    return GRLBWT_OK;
}
int grlbwt_cdebruijn_nodes(grlbwt_ctx *ctx, const grlbwt_cdebruijn *graph, uint64_t *dev_lo, uint64_t *dev_count, uint64_t *dev_mate_lo, uint64_t *dev_total,
                           uint32_t *dev_degree0, uint32_t *dev_degree1, uint64_t *dev_unitig, uint64_t *dev_rank, uint8_t *dev_orient, uint64_t capacity) {
    if (!ctx || !graph || !(graph->g32 || graph->g64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (graph->g32) grl32::Image::cdebruijn_nodes(*graph->g32, dev_lo, dev_count, dev_mate_lo, dev_total, dev_degree0, dev_degree1, dev_unitig, dev_rank, dev_orient, capacity);
        else grl64::Image::cdebruijn_nodes(*graph->g64, dev_lo, dev_count, dev_mate_lo, dev_total, dev_degree0, dev_degree1, dev_unitig, dev_rank, dev_orient, capacity);
    });
}
int grlbwt_cdebruijn_links(grlbwt_ctx *ctx, const grlbwt_cdebruijn *graph, uint64_t *dev_end_offsets, uint64_t *dev_other, uint64_t *dev_weight,
                           uint64_t *dev_fwd_row, uint64_t *dev_fwd_count, uint64_t capacity) {
    if (!ctx || !graph || !(graph->g32 || graph->g64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (graph->g32) grl32::Image::cdebruijn_links(*graph->g32, dev_end_offsets, dev_other, dev_weight, dev_fwd_row, dev_fwd_count, capacity);
        else grl64::Image::cdebruijn_links(*graph->g64, dev_end_offsets, dev_other, dev_weight, dev_fwd_row, dev_fwd_count, capacity);
    });
}
int grlbwt_cdebruijn_unitigs(grlbwt_ctx *ctx, const grlbwt_cdebruijn *graph, const grlbwt_fm *fm, int cell_bytes, uint64_t *dev_node_offsets,
                             uint64_t *dev_nodes, void *dev_cells, uint64_t *dev_weight, uint8_t *dev_circular, uint64_t capacity_unitigs,
                             uint64_t capacity_nodes, uint64_t capacity_cells) {
    if (!ctx || !graph || !(graph->g32 || graph->g64)) return refuse(ctx);
    if (fm && (graph->g32 ? !fm->f32 : !fm->f64)) return refuse(ctx, "canonical de bruijn unitigs: not the index the graph was made from");
    return guarded(ctx, [&] {
        if (graph->g32) grl32::Image::cdebruijn_unitigs(*graph->g32, fm ? fm->f32.get() : nullptr, cell_bytes, dev_node_offsets, dev_nodes, dev_cells,
                                                        dev_weight, dev_circular, capacity_unitigs, capacity_nodes, capacity_cells);
        else grl64::Image::cdebruijn_unitigs(*graph->g64, fm ? fm->f64.get() : nullptr, cell_bytes, dev_node_offsets, dev_nodes, dev_cells, dev_weight,
                                             dev_circular, capacity_unitigs, capacity_nodes, capacity_cells);
    });
}

int grlbwt_select_create(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int cell_bytes, const uint64_t *dev_ids, uint64_t n_ids,
                         uint32_t select_flags, grlbwt_select **out) {
    if (out) *out = nullptr;
    if (!ctx || !dev_image || !out || (n_ids && !dev_ids)) return refuse(ctx);
    const uint32_t sample_bits = (select_flags >> 8) & 0xFFu;
    const bool keep = select_flags & GRLBWT_SELECT_KEEP, cps = select_flags & GRLBWT_SELECT_CHECKPOINTS;
    if ((select_flags & ~(GRLBWT_SELECT_KEEP | GRLBWT_SELECT_CHECKPOINTS | 0xFF00u)) || sample_bits > 20 || (!cps && sample_bits)) {
        ctx->err = "select: bad flags (the keep flag, the checkpoint flag and sample_bits are all there is; sample_bits is 0 or 1 to 20 and needs the checkpoint flag)";
        return GRLBWT_EINVAL;
    }
    return guarded(ctx, [&] {
        const uint64_t total = grl64::Image::image_total_symbols(dev_image, image_bytes);
        if (total >= kMergeRowLimit) throw prim::Error(GRLBWT_ERANGE, "select: 2^40 rows or more");
        const bool big = idx64_for(ctx, total);
        std::unique_ptr<grlbwt_select> sel(new grlbwt_select());
        if (big) {
            sel->s64.reset(new grl64::Image::ImageSelect());
            sel->s64->flags = select_flags;
            grl64::Image::select_create(dev_image, image_bytes, cell_bytes, dev_ids, n_ids, keep, cps, (int)sample_bits, *sel->s64);
        } else {
            sel->s32.reset(new grl32::Image::ImageSelect());
            sel->s32->flags = select_flags;
            grl32::Image::select_create(dev_image, image_bytes, cell_bytes, dev_ids, n_ids, keep, cps, (int)sample_bits, *sel->s32);
        }
        ctx->selects.push_back(sel.get());
        *out = sel.release();
    });
}
int grlbwt_select_destroy(grlbwt_ctx *ctx, grlbwt_select *sel) {
    if (!ctx) return GRLBWT_EINVAL;
    if (!sel) return GRLBWT_OK;
    auto it = std::find(ctx->selects.begin(), ctx->selects.end(), sel);
    if (it == ctx->selects.end()) { ctx->err = "select destroy: not a selection of this context"; return GRLBWT_EINVAL; }
    ctx->selects.erase(it);
    return guarded(ctx, [&] { prim::sync(); delete sel; });
}
int grlbwt_select_info_get(const grlbwt_select *sel, grlbwt_select_info *out) {
    if (!sel || !out || !(sel->s32 || sel->s64)) return GRLBWT_EINVAL;
    auto fill = [&](const auto &S, uint64_t idx_bytes) {
        out->n_syms_in = S.n_in; out->n_strings_in = S.k_in; out->n_runs_in = S.R_in; out->n_listed = S.n_listed;
        out->rows_marked = S.rows_marked; out->longest_walk = S.longest_walk;
        out->n_syms_out = S.n_out; out->n_strings_out = S.k_out; out->n_runs_out = S.R_out; out->out_bytes = S.out_bytes; out->sb = S.sb; out->fb = S.fb;
        out->separator = S.sepval; out->idx_bytes = idx_bytes; out->flags = S.flags;
        out->walk_lanes = S.lanes; out->lane_refills = S.refills;
        out->sample_bits = S.sample_bits; out->n_checkpoints = S.n_checkpoints; out->jump_rounds = S.jump_rounds;
        out->scratch_bytes = S.scratch_bytes; out->held_bytes = S.held_bytes();
    };
    if (sel->s32) fill(*sel->s32, 4); else fill(*sel->s64, 8);
    return GRLBWT_OK;
}
int grlbwt_select_emit(grlbwt_ctx *ctx, const grlbwt_select *sel, void *dev_out, uint64_t capacity_bytes) {
    if (!ctx || !sel || !dev_out || !(sel->s32 || sel->s64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (sel->s32) grl32::Image::select_emit(*sel->s32, (uint8_t *)dev_out, capacity_bytes);
        else grl64::Image::select_emit(*sel->s64, (uint8_t *)dev_out, capacity_bytes);
    });
}
int grlbwt_select_rows(grlbwt_ctx *ctx, const grlbwt_select *sel, uint64_t *dev_bits) {
    if (!ctx || !sel || !dev_bits || !(sel->s32 || sel->s64)) return refuse(ctx);
    return guarded(ctx, [&] {
        if (sel->s32) grl32::Image::select_rows(*sel->s32, dev_bits);
        else grl64::Image::select_rows(*sel->s64, dev_bits);
    });
}
int grlbwt_select_files(grlbwt_ctx *ctx, const char *path_in, const uint64_t *host_ids, uint64_t n_ids, int cell_bytes, uint32_t select_flags,
                        const char *path_out, grlbwt_select_info *info) {
    if (!ctx || !path_in || !path_out || (n_ids && !host_ids)) return refuse(ctx);
    grlbwt_select *sel = nullptr;
    int rc = guarded(ctx, [&] {
        RawText a;
        read_image_file(path_in, a);
        grl64::DBuf<uint64_t> ids(n_ids);
        prim::h2d(ids.p, host_ids, n_ids * 8);
        const int r = grlbwt_select_create(ctx, a.buf.p, a.n, cell_bytes, ids.p, n_ids, select_flags, &sel);
        if (r != GRLBWT_OK) throw prim::Error(r, ctx->err);
    });
    if (rc != GRLBWT_OK) return rc;
    rc = guarded(ctx, [&] {
        grlbwt_select_info si;
        grlbwt_select_info_get(sel, &si);
        grl64::DBuf<uint8_t> out(si.out_bytes);
        const int r = grlbwt_select_emit(ctx, sel, out.p, si.out_bytes);
        if (r != GRLBWT_OK) throw prim::Error(r, ctx->err);
        write_image(out.p, si.out_bytes, path_out);
        if (info) *info = si;
    });
    const std::string err = ctx->err;
    grlbwt_select_destroy(ctx, sel);
    if (rc != GRLBWT_OK) ctx->err = err;
    return rc;
}

int grlbwt_image_plain(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, void *dev_out_u8,
                       uint64_t capacity, int null_char, uint64_t *n_out) {
    if (!ctx || !dev_image || !dev_out_u8 || null_char > 255) return refuse(ctx);
    return guarded(ctx, [&] {
        const uint64_t total = grl64::Image::image_total_symbols(dev_image, image_bytes);
        if (total > capacity) throw prim::Error(GRLBWT_EINVAL, "grl2plain: output buffer too small");
        bool big = idx64_for(ctx, total);
        uint64_t n = big ? grl64::Image::image_plain(dev_image, image_bytes, (uint8_t *)dev_out_u8, capacity, null_char)
                         : grl32::Image::image_plain(dev_image, image_bytes, (uint8_t *)dev_out_u8, capacity, null_char);
        if (n_out) *n_out = n;
    });
}
int grlbwt_image_rle(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, void *dev_syms_u8, void *dev_lens_u32,
                     uint64_t capacity_runs, uint64_t *n_runs_out) {
    if (!ctx || !dev_image || !dev_syms_u8 || !dev_lens_u32) return refuse(ctx);
    return guarded(ctx, [&] {
        uint64_t r = grl64::Image::image_rle(dev_image, image_bytes, (uint8_t *)dev_syms_u8, (uint32_t *)dev_lens_u32, capacity_runs);
        if (n_runs_out) *n_runs_out = r;
    });
}
int grlbwt_image_stats_get(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, grlbwt_image_stats *out) {
    if (!ctx || !dev_image || !out) return refuse(ctx);
    return guarded(ctx, [&] {
        grl64::Image::ImageStats st;
        grl64::Image::image_stats(dev_image, image_bytes, st);
        out->n_runs = st.n_runs; out->sigma = st.sigma; out->text_size = st.text_size; out->min_run = st.min_run; out->max_run = st.max_run;
        out->fit1 = st.fit1; out->fit2 = st.fit2; out->fit3 = st.fit3;
        for (int c = 0; c < 256; c++) { out->runs_of[c] = st.runs_of[c]; out->freq_of[c] = st.freq_of[c]; }
        for (int i = 0; i < 9; i++) out->deciles[i] = st.deciles[i];
        out->non_maximal = st.non_maximal;
    });
}

int grlbwt_image_split_runs(grlbwt_ctx *ctx, const void *dev_image, uint64_t image_bytes, int bits, uint64_t block_size,
                            void *dev_out, uint64_t capacity_bytes, grlbwt_split_info *info) {
    if (!ctx || !dev_image || !dev_out) return refuse(ctx);
    return guarded(ctx, [&] {
        const uint64_t total = grl64::Image::image_total_symbols(dev_image, image_bytes);
        bool big = idx64_for(ctx, total);
        uint64_t v[6];
        if (big) {
            auto si = grl64::Image::image_split_runs(dev_image, image_bytes, bits, block_size, (uint8_t *)dev_out, capacity_bytes);
            v[0] = si.runs_before; v[1] = si.runs_after; v[2] = si.overflow_splits; v[3] = si.block_splits; v[4] = si.n_syms; v[5] = si.out_bytes;
        } else {
            auto si = grl32::Image::image_split_runs(dev_image, image_bytes, bits, block_size, (uint8_t *)dev_out, capacity_bytes);
            v[0] = si.runs_before; v[1] = si.runs_after; v[2] = si.overflow_splits; v[3] = si.block_splits; v[4] = si.n_syms; v[5] = si.out_bytes;
        }
        if (info) {
            info->runs_before = v[0]; info->runs_after = v[1]; info->overflow_splits = v[2]; info->block_splits = v[3];
            info->n_syms = v[4]; info->out_bytes = v[5];
            info->n_blocks = block_size ? (v[4] > 0 ? 1 + (v[4] - 1) / block_size : 0) : 0;
        }
    });
}

int grlbwt_memory_usage(const grlbwt_ctx *ctx, uint64_t *peak_live_bytes, uint64_t *reserved_bytes) {
    if (!ctx) return GRLBWT_EINVAL;
    if (peak_live_bytes) *peak_live_bytes = prim::pool_peak_bytes();
    if (reserved_bytes) *reserved_bytes = prim::pool_reserved_bytes();
    return GRLBWT_OK;
}

int grlbwt_dist_build(grlbwt_ctx *ctx, const grlbwt_comm *comm) {
    if (!HAS_ENG(ctx) || !comm || !comm->allgather || !comm->alltoallv || comm->size < 1 || comm->rank < 0 || comm->rank >= comm->size) return refuse(ctx);
    return guarded(ctx, [&] {
        if (ctx->e32) {
            grl32::Engine::Comm C;
            C.rank = comm->rank; C.size = comm->size; C.user = comm->user; C.ag = comm->allgather; C.a2a = comm->alltoallv;
            C.stream_ordered = (comm->flags & GRLBWT_COMM_STREAM_ORDERED) != 0;
            C.keep_parts = (comm->flags & GRLBWT_COMM_KEEP_PARTS) != 0;
            ctx->e32->dist_build(C);
        } else {
            grl64::Engine::Comm C;
            C.rank = comm->rank; C.size = comm->size; C.user = comm->user; C.ag = comm->allgather; C.a2a = comm->alltoallv;
            C.stream_ordered = (comm->flags & GRLBWT_COMM_STREAM_ORDERED) != 0;
            C.keep_parts = (comm->flags & GRLBWT_COMM_KEEP_PARTS) != 0;
            ctx->e64->dist_build(C);
        }
    });
}

// ---- grlbwt_comm over RCCL, inside the library ---------------------------------------------------------------------
#ifdef GRLBWT_PRIM_HIP
}   // extern "C"
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and prototypes only: librccl (573 MB) is loaded on first use, not linked
namespace {
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        // a librccl already mapped into the process (torch brings its own) is found by its soname
        for (const char *name : {"librccl.so.1", "librccl.so"}) { lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
        auto sym = [&](const char *n) { void *p = dlsym(lib, n); if (!p) err = std::string("librccl lacks ") + n; return p; };
        GetUniqueId = (decltype(GetUniqueId))sym("ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))sym("ncclCommInitRank");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        AllGather = (decltype(AllGather))sym("ncclAllGather");
        Send = (decltype(Send))sym("ncclSend");
        Recv = (decltype(Recv))sym("ncclRecv");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (!err.empty()) { dlclose(lib); lib = nullptr; return false; }
        return true;
    }
};
RcclApi &rccl() { static RcclApi a; return a; }
struct RcclState { ncclComm_t comm = nullptr; int rank = 0, size = 1; };
// stream-ordered callbacks: everything is enqueued on the engine's stream and nobody waits on the host
int rccl_allgather(void *user, const void *send, void *recv, uint64_t bytes) {
    RcclState *S = (RcclState *)user;
    return rccl().AllGather(send, recv, (size_t)bytes, ncclUint8, S->comm, prim::rt().stream) == ncclSuccess ? 0 : 1;
}
int rccl_alltoallv(void *user, const void *send, const uint64_t *sb, const uint64_t *so, void *recv, const uint64_t *rb, const uint64_t *ro) {
    RcclState *S = (RcclState *)user;
    RcclApi &A = rccl();
    bool ok = A.GroupStart() == ncclSuccess;
    for (int g = 0; g < S->size && ok; g++) {        // one grouped send/recv per peer: direct xGMI writes, no staging
        if (sb[g]) ok = A.Send((const char *)send + so[g], (size_t)sb[g], ncclUint8, g, S->comm, prim::rt().stream) == ncclSuccess;
        if (ok && rb[g]) ok = A.Recv((char *)recv + ro[g], (size_t)rb[g], ncclUint8, g, S->comm, prim::rt().stream) == ncclSuccess;
    }
    return (A.GroupEnd() == ncclSuccess && ok) ? 0 : 1;
}
}   // namespace
extern "C" {
int grlbwt_rccl_unique_id(void *id128) {
    if (!id128) return GRLBWT_EINVAL;
    if (!rccl().load()) return GRLBWT_EDEVICE;
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) return GRLBWT_EINTERNAL;
    static_assert(sizeof id == GRLBWT_RCCL_ID_BYTES, "ncclUniqueId size");
    memcpy(id128, &id, sizeof id);
    return GRLBWT_OK;
}
int grlbwt_rccl_comm_create(grlbwt_ctx *ctx, const void *id128, int rank, int size, grlbwt_comm *comm) {
    if (!ctx || !id128 || !comm || size < 1 || rank < 0 || rank >= size) return refuse(ctx);
    return guarded(ctx, [&] {
        if (!rccl().load()) throw prim::Error(GRLBWT_EDEVICE, rccl().err);
        ncclUniqueId id;
        memcpy(&id, id128, sizeof id);
        std::unique_ptr<RcclState> S(new RcclState());
        S->rank = rank; S->size = size;
        ncclResult_t r = rccl().CommInitRank(&S->comm, size, id, rank);          // collective over all ranks; uses the current device
        if (r != ncclSuccess) throw prim::Error(GRLBWT_EINTERNAL, std::string("ncclCommInitRank: ") + rccl().GetErrorString(r));
        comm->rank = rank; comm->size = size; comm->user = S.release();
        comm->allgather = rccl_allgather; comm->alltoallv = rccl_alltoallv;
        comm->flags = GRLBWT_COMM_STREAM_ORDERED;
    });
}
int grlbwt_rccl_comm_destroy(grlbwt_comm *comm) {
    if (!comm || comm->allgather != rccl_allgather || !comm->user) return GRLBWT_EINVAL;
    RcclState *S = (RcclState *)comm->user;
    try { prim::sync(); } catch (...) {}
    if (S->comm) rccl().CommDestroy(S->comm);
    delete S;
    comm->user = nullptr; comm->allgather = nullptr; comm->alltoallv = nullptr;
    return GRLBWT_OK;
}
#else   // the tests' serial stand-in has no device and no RCCL
int grlbwt_rccl_unique_id(void *) { return GRLBWT_EDEVICE; }
int grlbwt_rccl_comm_create(grlbwt_ctx *, const void *, int, int, grlbwt_comm *) { return GRLBWT_EDEVICE; }
int grlbwt_rccl_comm_destroy(grlbwt_comm *) { return GRLBWT_EDEVICE; }
#endif

int grlbwt_profile_enable(grlbwt_ctx *ctx, int on) {
    if (!ctx) return GRLBWT_EINVAL;
    return guarded(ctx, [&] {
        prim::sync();
        prim::rt().prof.clear();
        prim::rt().profile = on != 0;
    });
}
int grlbwt_profile_dump(grlbwt_ctx *ctx, char *buf, uint64_t capacity) {
    if (!ctx || !buf || capacity == 0) return refuse(ctx);
    return guarded(ctx, [&] {
        prim::sync();
        std::string s;
        for (const auto &kv : prim::rt().prof) {
            char line[256];
            snprintf(line, sizeof line, "%s %llu %.6f %llu\n", kv.first.c_str(), (unsigned long long)kv.second.launches, kv.second.ms,
                     (unsigned long long)kv.second.bytes);
            s += line;
        }
        size_t n = s.size() < capacity - 1 ? s.size() : (size_t)capacity - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    });
}

int grlbwt_selftest(grlbwt_ctx *ctx, uint64_t n, uint64_t seed) {
    if (!ctx) return GRLBWT_EINVAL;
    int res = 0;
    int rc = guarded(ctx, [&] { res = selftest(n, seed); });
    return rc != GRLBWT_OK ? rc - 1000 : res;
}

}   // extern "C"
