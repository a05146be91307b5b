#!/usr/bin/env python3
"""grlbwt_docs_* -- which strings lie behind row ranges of an FM index, and how many -- on the 101 MB read collection of the other
tools/gpu_fm_*.py (1,000,000 x 100 bp uniform reads, grlbwt_amd/workloads.py).

Written to --out (profiles/fm_docs/docs.txt):
  create   grlbwt_docs_create on an index without checkpoints (form 0) and with them (form 1, sample_bits 4), with and without
           GRLBWT_DOCS_OCCURRENCES: median time, held_bytes, scratch_bytes, walk_steps.  (grlbwt_fm_sa's time for the same
           indexes is in profiles/fm_sa/sa.txt.)
  queries  two batches of ranges, on the form 0 index:
             kmers     the (lo, lo + count) ranges of grlbwt_fm_kmers at k = 31 with min_count = 2
             prefixes  the ranges grlbwt_fm_count gives for the first 20 cells of 2^17 reads
           and, because these reads are uniformly random (no 31-mer occurs twice, a 20-cell prefix occurs once), the same two kinds
           at k = 12 and at 10 cells, where a range holds rows of several strings
           count, list with every array (a handle with occurrences) and list without dev_occ, against the ROUTE WITHOUT THE CALL:
           grlbwt_fm_locate of every range row, then a unique of (range, string) in torch on the device.
  forms    with --lib pointing at the development build (tools/build_dev.sh) the tile kernels take turns with the generic form
           (GRLBWT_DEV_DOCS_TILE=f: a search per range row and per entry).
After a warm-up of every call the variants take turns inside each repetition; every timing is a host clock around work that ends
in a device synchronise; medians, fastest and slowest are written.  Nothing about the ratios is fixed in advance.

Checked on the way: count's numbers equal the route's per range; list's offsets are their scan; both forms write the same.

Usage: python tools/gpu_fm_docs.py [--lib tools/_build/libgrlbwt_dev.so] [--out profiles/fm_docs/docs.txt] [--reps 5] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 31
PREFIX = 20
N_PREFIXES = 1 << 17
K_SHORT = 12
PREFIX_SHORT = 10


def set_form(value):
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    if value is None:
        os.environ.pop("GRLBWT_DEV_DOCS_TILE", None)
    else:
        os.environ["GRLBWT_DEV_DOCS_TILE"] = value


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def line(label, ts, extra=""):
    ts = sorted(ts)
    return "  %-34s: median %9.3f ms  min %9.3f  max %9.3f%s" % (label, statistics.median(ts) * 1e3, ts[0] * 1e3, ts[-1] * 1e3, extra)


def measure(args, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
    lib = os.path.abspath(args.lib) if args.lib else g.build_hip()
    forms = (("tile", None), ("generic", "f")) if args.lib else (("tile", None),)
    div = 16 if args.small else 1
    n_reads = 1000000 // div
    text = workloads.uniform_reads_torch(n_reads, 100, device="cuda:0")
    torch.cuda.synchronize()
    i64 = dict(dtype=torch.int64, device="cuda:0")
    set_form(None)
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        # ---- create, both forms
        for bits in (None, 4):
            kw = {} if bits is None else dict(checkpoints=True, sample_bits=bits)
            with engine.FmIndex(ctx, image_ptr, nb, locate=True, **kw) as fm:
                info = fm.info()
                say("== create, %s: %d rows, %d strings, %d runs, index %d bytes, idx_bytes %d"
                    % ("form 0 (no checkpoints)" if bits is None else "form 1 (sample_bits %d)" % bits, info["n_syms"], info["n_strings"], runs,
                       info["index_bytes"], info["idx_bytes"]))
                for occ in (False, True):
                    fm.documents(occurrences=occ).close()        # warm-up
                    ts = []
                    for _ in range(args.reps):
                        box = []
                        ts.append(timed(torch, lambda: box.append(fm.documents(occurrences=occ))))
                        di = box[0].info()
                        box[0].close()
                    say(line("with occurrences" if occ else "without occurrences", ts,
                             "  held %d bytes, scratch %d bytes, %d LF steps, %d sort bits" % (di["held_bytes"], di["scratch_bytes"], di["walk_steps"], di["sort_bits"])))
        # ---- queries, on the form 0 index
        with engine.FmIndex(ctx, image_ptr, nb, locate=True) as fm:
            n, k = fm.info()["n_syms"], fm.info()["n_strings"]
            npre = min(N_PREFIXES, n_reads)

            def kmer_ranges(kk):
                m = fm.kmers_raw(kk, min_count=2)
                klo, kcnt = torch.zeros(m, **i64), torch.zeros(m, **i64)
                torch.cuda.synchronize()
                if m:
                    assert fm.kmers_raw(kk, min_count=2, lo_ptr=klo.data_ptr(), count_ptr=kcnt.data_ptr(), capacity=m) == m
                torch.cuda.synchronize()
                return "kmers: k = %d, min_count = 2" % kk, klo, klo + kcnt

            def prefix_ranges(cells_each):
                cells = text.view(n_reads, 101)[:npre, :cells_each].contiguous()
                off = torch.arange(npre + 1, **i64) * cells_each
                plo, phi = torch.zeros(npre, **i64), torch.zeros(npre, **i64)
                torch.cuda.synchronize()
                fm.count(cells.data_ptr(), 1, off.data_ptr(), npre, plo.data_ptr(), phi.data_ptr())
                torch.cuda.synchronize()
                return "prefixes: %d cells of %d reads" % (cells_each, npre), plo, phi

            # the two batches asked for, and -- the reads are uniformly random: no 31-mer occurs twice and a 20-cell prefix occurs
            # once -- the same two kinds at lengths where a range holds rows of several strings
            batches = (kmer_ranges(K), prefix_ranges(PREFIX), kmer_ranges(K_SHORT), prefix_ranges(PREFIX_SHORT))
            with fm.documents(occurrences=True) as docs, fm.documents() as plain:
                for name, lo, hi in batches:
                    nr = lo.numel()
                    size = hi - lo
                    rows_total = int(size.sum())
                    nd = torch.zeros(nr, **i64)
                    torch.cuda.synchronize()
                    total = docs.count(lo.data_ptr(), hi.data_ptr(), nr, nd.data_ptr())
                    qi = docs.info()
                    say("== %s: %d ranges, %d range rows, %d documents, largest range %d, most documents %d, tile %d"
                        % (name, nr, qi["n_range_rows"], total, qi["largest_range"], qi["most_docs"], qi["tile_entries"]))
                    assert qi["n_range_rows"] == rows_total and qi["n_entries"] == total
                    if nr == 0:
                        say("  (no range: nothing to time)")
                        continue
                    eoff = torch.zeros(nr + 1, **i64)
                    arr = [torch.zeros(max(total, 1), **i64) for _ in range(4)]

                    def do_count(form, h=docs):
                        set_form(form)
                        return timed(torch, lambda: h.count(lo.data_ptr(), hi.data_ptr(), nr, nd.data_ptr()))

                    def do_list(form, h, occ):
                        set_form(form)
                        return timed(torch, lambda: h.list(lo.data_ptr(), hi.data_ptr(), nr, eoff.data_ptr(), arr[0].data_ptr(), total, arr[1].data_ptr(),
                                                           arr[2].data_ptr() if occ else None, arr[3].data_ptr()))

                    def route():
                        """the route without the call: every range row located, then a unique of (range, string) on the device"""
                        def run():
                            rid = torch.repeat_interleave(torch.arange(nr, **i64), size)
                            start = torch.cumsum(size, 0) - size
                            rows = lo[rid] + (torch.arange(rows_total, **i64) - start[rid])
                            s, o = torch.zeros(rows_total, **i64), torch.zeros(rows_total, **i64)
                            torch.cuda.synchronize()             # (the library runs on its own stream: torch's work comes first)
                            fm.locate(rows.data_ptr(), rows_total, engine.UINT64_MAX, s.data_ptr(), o.data_ptr())
                            torch.cuda.synchronize()
                            pairs = torch.unique(rid * k + s)
                            route.ndocs = torch.bincount(pairs // k, minlength=nr)
                        return timed(torch, run)

                    calls = [("route without the call", route)]
                    for label, form in forms:
                        calls += [("count, %s" % label, lambda form=form: do_count(form)),
                                  ("list, all arrays, %s" % label, lambda form=form: do_list(form, docs, True)),
                                  ("list without dev_occ, %s" % label, lambda form=form: do_list(form, plain, False))]
                    ref = None
                    for label, fn in calls:                      # warm-up, and every variant writes the same
                        nd.zero_(); eoff.zero_()
                        for a in arr:
                            a.zero_()
                        fn()
                        if label.startswith("route"):
                            continue
                        if label.startswith("count"):
                            assert torch.equal(nd, route.ndocs), "count differs from the route without the call"
                        else:
                            assert torch.equal(eoff[1:] - eoff[:-1], route.ndocs) and int(eoff[-1]) == total
                            got = [a.clone() for a in arr]
                            if label.startswith("list, all"):
                                if ref is None:
                                    ref = got
                                assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
                                assert int(got[2].sum()) == rows_total          # every range row is an occurrence of one document
                    times = {label: [] for label, _ in calls}
                    for _ in range(args.reps):
                        for label, fn in calls:
                            times[label].append(fn())
                    set_form(None)
                    base = statistics.median(times[calls[0][0]])
                    for label, _ in calls:
                        med = statistics.median(times[label])
                        say(line(label, times[label], "  route / this = %7.2f  %7.2f G range rows/s" % (base / med, rows_total / med / 1e9)))
                    del arr, eoff, nd, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="a development library (tools/build_dev.sh): the generic form is measured too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_docs", "docs.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a sixteenth of the collection")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    torch.zeros(1, device="cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("grlbwt_docs_* on the 101 MB uniform reads, on %s%s%s"
        % (torch.cuda.get_device_name(0), "; the tile kernels (default) against the generic form (GRLBWT_DEV_DOCS_TILE=f)" if args.lib else "",
           "; the collection cut to a sixteenth (--small)" if args.small else ""))
    measure(args, say)


if __name__ == "__main__":
    main()
