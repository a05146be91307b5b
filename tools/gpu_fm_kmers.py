#!/usr/bin/env python3
"""grlbwt_fm_kmers on images of read collections at k = 21 and 31: the whole table (cells, lo, count) and a spectrum of 256 bins.

ONE leg per invocation (--leg); the tool starts no child process.  Every leg is its own command under `timeout`, chained with `&&`:
    timeout -k 10 400 python tools/gpu_fm_kmers.py --leg reads101 --lib tools/_build/libgrlbwt_dev.so --route-b &&
    timeout -k 10 600 python tools/gpu_fm_kmers.py --leg reads1g --lib tools/_build/libgrlbwt_dev.so --route-b --append
Legs (grlbwt_amd/workloads.py, as tools/gpu_fm_lcp.py):
  reads101  1,000,000 x 100 bp uniform reads (101 MB)
  reads1g   6,622,517 x 150 bp reads sampled from a 33 Mbp genome (1 GB)

Per leg and k: a sizing call (no arrays), then the filling call timed `--reps` times; with a development library (--lib, built by
tools/build_dev.sh) the tile decode and the generic one (GRLBWT_DEV_KMER_DECODE=f: for_each_set_bit, one lane per entry storing its
own cells) take turns inside each repetition and must write the same bytes.  One more call of each form runs under the library's
profile: the kernels' times, grouped into the LCP passes, the length passes, the counting (heads, word list, spectrum, selection)
and the decode.  Written: n_distinct, n_windows, the passes, the call's median, the groups, the decode's forward steps per second
and bytes written per second.

--route-b: the route without this call, timed once: grlbwt_fm_lcp with max_lcp = k and 1-byte values into a device array, the
array downloaded, the boundaries found on the host, every boundary row located and k cells extracted from its position on an
index made with GRLBWT_FM_LOCATE | GRLBWT_FM_EXTRACT; the ranges that come back with k cells, the k-th not the separator, are the
k-mers.  Their number from the positions and the strings' lengths alone must be n_distinct.

Usage: python tools/gpu_fm_kmers.py --leg reads101|reads1g [--lib LIB] [--route-b] [--out profiles/fm_kmers/kmers.txt] [--append]
                                    [--reps 3] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("reads101", "reads1g")
KS = (21, 31)
GROUPS = (("lcp passes", ("lcp.",)), ("length passes", ("kmer.lengths", "kmer.suffixes", "kmer.terminators")), ("decode", ("kmer.decode",)),
          ("counting", ("kmer.",)))


def set_form(value):
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    if value is None:
        os.environ.pop("GRLBWT_DEV_KMER_DECODE", None)
    else:
        os.environ["GRLBWT_DEV_KMER_DECODE"] = value


def make_text(workloads, leg, small):
    div = 16 if small else 1
    if leg == "reads101":
        return "101 MB uniform reads", workloads.uniform_reads_torch(1000000 // div, 100, device="cuda:0")
    return "1 GB sampled reads", workloads.sampled_reads_torch(6622517 // div, 150, 33000000 // div, device="cuda:0")


def grouped(prof):
    out = {g: 0.0 for g, _ in GROUPS}
    for name, (_, ms, _) in prof.items():
        for g, prefixes in GROUPS:
            if any(name.startswith(p) for p in prefixes):
                out[g] += ms
                break
    return out


def route_b(torch, np, ctx, engine, image_ptr, nb, k, n, say):
    with engine.FmIndex(ctx, image_ptr, nb, locate=True, extract=True) as fm:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lcp = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()                         # (the library runs on its own stream: torch's fills come first)
        fm.lcp(k, 1, lcp.data_ptr(), want_hist=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = lcp.cpu().numpy()
        rows = np.flatnonzero(host < k).astype(np.uint64)
        m = len(rows)
        t2 = time.perf_counter()
        drows = torch.from_numpy(rows.view(np.int64)).to("cuda:0")
        s, o = torch.zeros(m, dtype=torch.int64, device="cuda:0"), torch.zeros(m, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        fm.locate(drows.data_ptr(), m, engine.UINT64_MAX, s.data_ptr(), o.data_ptr())
        end = o + k
        off = torch.zeros(m + 1, dtype=torch.int64, device="cuda:0")
        cells = torch.zeros(m * k, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        fm.extract(s.data_ptr(), o.data_ptr(), end.data_ptr(), m, 1, cells.data_ptr(), m * k, off.data_ptr())
        torch.cuda.synchronize()
        whole = (off[1:] - off[:-1]) == k                # k cells came back: a k-mer unless the k-th is the string's separator
        sep = fm.info()["separator"]
        full = int((whole & (cells[(off[1:] - 1).clamp(min=0)] != sep)).sum())
        t3 = time.perf_counter()
        slen = torch.zeros(fm.info()["n_strings"], dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        fm.string_lengths(slen.data_ptr())
        torch.cuda.synchronize()
        by_len = int((o + k <= slen[s] - 1).sum())       # the same from the positions and the strings' lengths alone
    say("  route without the call: lcp %.1f ms, download and boundaries on the host %.1f ms (%d rows), locate + extract %.1f ms: %.1f ms, %d k-mers"
        " (%d by the positions and the lengths)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, m, (t3 - t2) * 1e3, (t3 - t0) * 1e3, full, by_len))
    return by_len


def measure(leg, args, say):
    import numpy as np
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
    lib = os.path.abspath(args.lib) if args.lib else g.build_hip()
    forms = (("tile", None), ("generic", "f")) if args.lib else (("tile", None),)
    name, text = make_text(workloads, leg, args.small)
    torch.cuda.synchronize()
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        set_form(None)
        with engine.FmIndex(ctx, image_ptr, nb) as fm:
            info = fm.info()
            n = info["n_syms"]
            say("== %s: %d cells, %d strings, %d runs, idx_bytes %d" % (name, n, info["n_strings"], runs, info["idx_bytes"]))
            for k in KS:
                spec = np.zeros(256, dtype=np.uint64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = fm.kmers_raw(k, spectrum=spec)
                t_size = time.perf_counter() - t0
                ki = fm.kmer_info()
                assert int(spec.sum()) == ki["n_distinct"] == m
                cells = torch.zeros(m * k, dtype=torch.uint8, device="cuda:0")
                lo, cnt = torch.zeros(m, dtype=torch.int64, device="cuda:0"), torch.zeros(m, dtype=torch.int64, device="cuda:0")

                def call(form):
                    set_form(form)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = fm.kmers_raw(k, cell_bytes=1, cells_ptr=cells.data_ptr(), lo_ptr=lo.data_ptr(), count_ptr=cnt.data_ptr(), capacity=m, spectrum=spec)
                    torch.cuda.synchronize()
                    assert got == m
                    return time.perf_counter() - t0

                ref = None
                for label, form in forms:                    # warm-up, and both forms write the same
                    cells.zero_(); lo.zero_(); cnt.zero_()
                    call(form)
                    got = (cells.clone(), lo.clone(), cnt.clone())
                    if ref is None:
                        ref = got
                    assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
                assert int(cnt.sum()) == ki["n_windows"] and bool((lo[1:] > lo[:-1]).all())
                times = {label: [] for label, _ in forms}
                for _ in range(args.reps):
                    for label, form in forms:
                        times[label].append(call(form))
                ki = fm.kmer_info()
                say("k = %d: %d distinct k-mers of %d windows, largest count %d; %d LCP passes + %d length passes; scratch %d bytes; sizing call %.1f ms"
                    % (k, ki["n_distinct"], ki["n_windows"], ki["largest_count"], ki["passes"], ki["length_passes"], ki["scratch_bytes"], t_size * 1e3))
                for label, form in forms:
                    ctx.profile_enable(True)
                    call(form)
                    gr = grouped(ctx.profile())
                    ctx.profile_enable(False)
                    ts = sorted(times[label])
                    dec = gr["decode"] / 1e3
                    say("  %-7s: call median %9.2f ms  min %9.2f  max %9.2f | kernels: lcp passes %8.2f, length passes %7.2f, counting %7.2f, decode %8.3f ms"
                        " -> %6.2f G steps/s, %6.1f GB/s written"
                        % (label, statistics.median(ts) * 1e3, ts[0] * 1e3, ts[-1] * 1e3, gr["lcp passes"], gr["length passes"], gr["counting"],
                           gr["decode"], ki["forward_steps"] / dec / 1e9 if dec > 0 else 0.0, m * (k + 16) / dec / 1e9 if dec > 0 else 0.0))
                set_form(None)
                del cells, lo, cnt, ref, got
                if args.route_b:
                    assert route_b(torch, np, ctx, engine, image_ptr, nb, k, n, say) == ki["n_distinct"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--lib", default=None, help="a development library (tools/build_dev.sh): the generic decode is measured too")
    ap.add_argument("--route-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_kmers", "kmers.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a sixteenth of every collection")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    torch.zeros(1, device="cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = open(args.out).read().splitlines() if args.append and os.path.exists(args.out) else []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not lines:
        say("grlbwt_fm_kmers: the whole table and a spectrum of 256 bins, the tile decode (default) against the generic one "
            "(GRLBWT_DEV_KMER_DECODE=f) on %s%s" % (torch.cuda.get_device_name(0), "; collections cut to a sixteenth (--small)" if args.small else ""))
    measure(args.leg, args, say)


if __name__ == "__main__":
    main()
