#!/usr/bin/env python3
"""grlbwt_fm_kmers_canonical on images of read collections at k = 31, each collection as built and with the reverse complement of
every read appended (what the command line's -R writes): the whole table (cells, lo, count, mate_lo, total) and a spectrum of 256 bins.

ONE leg per invocation (--leg); the tool starts no child process.  Every leg is its own command under `timeout`, chained with `&&`:
    timeout -k 10 300 python tools/gpu_fm_ckmers.py --leg reads101 --lib tools/_build/libgrlbwt_dev.so --route-b &&
    timeout -k 10 300 python tools/gpu_fm_ckmers.py --leg reads101R --lib tools/_build/libgrlbwt_dev.so --route-b --append && ...
Legs (grlbwt_amd/workloads.py, as tools/gpu_fm_kmers.py; an R behind the name: both strands):
  reads101  1,000,000 x 100 bp uniform reads (101 MB)
  reads1g   6,622,517 x 150 bp reads sampled from a 33 Mbp genome (1 GB)

Per leg: a sizing call (no arrays), then grlbwt_fm_kmers (cells, lo, count) and grlbwt_fm_kmers_canonical (all five arrays) take
turns inside each of `--reps` repetitions; with a development library (--lib, built by tools/build_dev.sh) the generic mate pass
(GRLBWT_DEV_KMER_MATES=f: for_each_set_bit over the heads, no top level, the table in memory) takes its turn too and must write
the same bytes.  One more call of each form runs under the library's profile: the mate pass's kernel time and its backward steps
per second.  Written: the medians, the classes, the step counters.

--route-b: the route without the call, timed once: grlbwt_fm_kmers with cells, the table downloaded, the reverse complements made
on the host, grlbwt_fm_count of all of them, the pairing (mate = the range's lo where it is not empty) on the host.  Its number of
classes must be the call's.

Usage: python tools/gpu_fm_ckmers.py --leg reads101|reads101R|reads1g|reads1gR [--lib LIB] [--route-b] [--out profiles/fm_ckmers/ckmers.txt]
                                     [--append] [--reps 3] [--small] [--k 31]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("reads101", "reads101R", "reads1g", "reads1gR")


def set_form(value):
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    if value is None:
        os.environ.pop("GRLBWT_DEV_KMER_MATES", None)
    else:
        os.environ["GRLBWT_DEV_KMER_MATES"] = value


def make_text(torch, workloads, leg, small):
    div = 16 if small else 1
    if leg.startswith("reads101"):
        name, n_reads, length = "101 MB uniform reads", 1000000 // div, 100
        text = workloads.uniform_reads_torch(n_reads, length, device="cuda:0")
    else:
        name, n_reads, length = "1 GB sampled reads", 6622517 // div, 150
        text = workloads.sampled_reads_torch(n_reads, length, 33000000 // div, device="cuda:0")
    if leg.endswith("R"):
        comp = torch.arange(256, dtype=torch.uint8, device="cuda:0")
        for a, b in ((65, 84), (67, 71)):
            comp[a], comp[b] = b, a
        view = text.view(n_reads, length + 1)
        rc = view.clone()
        rc[:, :length] = comp[view[:, :length].flip(1).long()]
        text = torch.cat([text, rc.reshape(-1)])
        name += ", both strands"
    return name, text


def route_b(torch, np, fm, k, n_distinct, say):
    comp = np.arange(256, dtype=np.uint8)
    for a, b in ((65, 84), (67, 71)):
        comp[a], comp[b] = b, a
    m = n_distinct
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cells = torch.zeros(m * k, dtype=torch.uint8, device="cuda:0")
    lo, cnt = torch.zeros(m, dtype=torch.int64, device="cuda:0"), torch.zeros(m, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert fm.kmers_raw(k, cell_bytes=1, cells_ptr=cells.data_ptr(), lo_ptr=lo.data_ptr(), count_ptr=cnt.data_ptr(), capacity=m) == m
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host = cells.cpu().numpy().reshape(m, k)
    rc = np.ascontiguousarray(comp[host[:, ::-1]])
    t2 = time.perf_counter()
    drc = torch.from_numpy(rc.reshape(-1)).to("cuda:0")
    off = torch.arange(0, (m + 1) * k, k, dtype=torch.int64, device="cuda:0")
    a, b = torch.zeros(m, dtype=torch.int64, device="cuda:0"), torch.zeros(m, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    fm.count(drc.data_ptr(), 1, off.data_ptr(), m, a.data_ptr(), b.data_ptr())
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    hlo, ha, hb = lo.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()
    classes = int(np.count_nonzero((ha >= hb) | (ha >= hlo)))      # no mate, or one at or behind the k-mer
    t4 = time.perf_counter()
    say("  route without the call: grlbwt_fm_kmers %.1f ms, download and reverse complements on the host %.1f ms, upload and grlbwt_fm_count "
        "of %d patterns %.1f ms, pairing on the host %.1f ms: %.1f ms, %d classes"
        % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, m, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (t4 - t0) * 1e3, classes))
    return classes


def measure(leg, args, say):
    import numpy as np
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
    lib = os.path.abspath(args.lib) if args.lib else g.build_hip()
    forms = (("tickets", None), ("generic", "f")) if args.lib else (("tickets", None),)
    k = args.k
    name, text = make_text(torch, workloads, leg, args.small)
    torch.cuda.synchronize()
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        set_form(None)
        with engine.FmIndex(ctx, image_ptr, nb) as fm:
            info = fm.info()
            say("== %s: %d cells, %d strings, %d runs, idx_bytes %d" % (name, info["n_syms"], info["n_strings"], runs, info["idx_bytes"]))
            spec = np.zeros(256, dtype=np.uint64)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = fm.canonical_kmers_raw(k, spectrum=spec)
            t_size = time.perf_counter() - t0
            ci = fm.canonical_kmer_info()
            assert int(spec.sum()) == ci["n_classes"] == m and ci["n_distinct"] == 2 * ci["n_paired"] + ci["n_palindromes"] + ci["n_single"]
            nd = ci["n_distinct"]
            cells = torch.zeros(nd * k, dtype=torch.uint8, device="cuda:0")
            cols = [torch.zeros(nd, dtype=torch.int64, device="cuda:0") for _ in range(4)]

            def plain():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fm.kmers_raw(k, cell_bytes=1, cells_ptr=cells.data_ptr(), lo_ptr=cols[0].data_ptr(), count_ptr=cols[1].data_ptr(), capacity=nd,
                                   spectrum=spec)
                torch.cuda.synchronize()
                assert got == nd
                return time.perf_counter() - t0

            def call(form):
                set_form(form)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fm.canonical_kmers_raw(k, cell_bytes=1, cells_ptr=cells.data_ptr(), lo_ptr=cols[0].data_ptr(), count_ptr=cols[1].data_ptr(),
                                             mate_lo_ptr=cols[2].data_ptr(), total_ptr=cols[3].data_ptr(), capacity=m, spectrum=spec)
                torch.cuda.synchronize()
                assert got == m
                return time.perf_counter() - t0

            plain()                                          # warm-up
            ref = None
            for label, form in forms:                        # warm-up, and both forms write the same
                cells.zero_()
                for c in cols:
                    c.zero_()
                call(form)
                got = [cells[:m * k].clone()] + [c[:m].clone() for c in cols]
                if ref is None:
                    ref = got
                assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
            assert int(ref[4].sum()) == ci["n_windows"] and bool((ref[1][1:] > ref[1][:-1]).all())
            del ref, got
            times = {label: [] for label, _ in forms}
            times["grlbwt_fm_kmers"] = []
            for _ in range(args.reps):
                times["grlbwt_fm_kmers"].append(plain())
                for label, form in forms:
                    times[label].append(call(form))
            ci = fm.canonical_kmer_info()
            say("k = %d: %d distinct k-mers of %d windows in %d classes: %d paired, %d palindromes, %d single (%d without complement); largest total %d; "
                "scratch %d bytes; sizing call %.1f ms"
                % (k, nd, ci["n_windows"], ci["n_classes"], ci["n_paired"], ci["n_palindromes"], ci["n_single"], ci["n_no_complement"],
                   ci["largest_total"], ci["scratch_bytes"], t_size * 1e3))
            say("  mate pass: %d walks, %d backward steps (%.2f per k-mer), %d forward steps with the decode's %d"
                % (ci["mate_walks"], ci["backward_steps"], ci["backward_steps"] / max(nd, 1), ci["forward_steps"], m * k))
            ts = sorted(times["grlbwt_fm_kmers"])
            base = statistics.median(ts)
            say("  %-15s: call median %9.2f ms  min %9.2f  max %9.2f (%d entries)" % ("grlbwt_fm_kmers", base * 1e3, ts[0] * 1e3, ts[-1] * 1e3, nd))
            for label, form in forms:
                ctx.profile_enable(True)
                call(form)
                prof = ctx.profile()
                ctx.profile_enable(False)
                mates = sum(ms for name, (_, ms, _) in prof.items() if name.startswith("ckmer.mates"))
                other = sum(ms for name, (_, ms, _) in prof.items() if name.startswith("ckmer.") and not name.startswith("ckmer.mates"))
                ts = sorted(times[label])
                med = statistics.median(ts)
                say("  %-15s: call median %9.2f ms  min %9.2f  max %9.2f (%.2f x grlbwt_fm_kmers) | kernels: mate pass %9.2f ms -> %5.2f G backward steps/s, "
                    "the other class kernels %7.2f ms"
                    % (label, med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, med / base, mates, ci["backward_steps"] / (mates / 1e3) / 1e9 if mates > 0 else 0.0,
                       other))
            set_form(None)
            del cells, cols
            if args.route_b:
                assert route_b(torch, np, fm, k, nd, say) == ci["n_classes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--lib", default=None, help="a development library (tools/build_dev.sh): the generic mate pass is measured too")
    ap.add_argument("--route-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_ckmers", "ckmers.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=31)
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
        say("grlbwt_fm_kmers_canonical: the whole table and a spectrum of 256 bins against grlbwt_fm_kmers on the same index; the ticket kernel of "
            "the mate pass (default) against the generic form (GRLBWT_DEV_KMER_MATES=f) on %s%s"
            % (torch.cuda.get_device_name(0), "; collections cut to a sixteenth (--small)" if args.small else ""))
    measure(args.leg, args, say)


if __name__ == "__main__":
    main()
