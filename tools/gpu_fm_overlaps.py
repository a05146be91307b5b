#!/usr/bin/env python3
"""grlbwt_fm_overlaps_of / grlbwt_fm_overlaps / grlbwt_fm_overlap_targets on the 1 GB sampled-read workload (6,622,517 reads of
150 bp from a 33 Mbp genome, grlbwt_amd/workloads.py).

One process, no children.  Build the image, make one index with the locate structures, then time
  overlaps_of   every read by number at min_len 50, without GRLBWT_FM_OVERLAP_PROPER and with it;
  overlaps      the same reads given as cells (their text without the separators): the difference is the price of reading the
                text from the index by the LF walk;
  targets       the hit list of the first call expanded into string numbers, and one range of n_strings;
  grlbwt_fm_count on 2^20 patterns of 32 cells beside them: the yardstick for one backward step (profiles/fm_match/match.txt).
With --lib pointing at the development build (tools/build_dev.sh) the tile kernel of the targets also takes turns with the form
it replaces, the for_each with a search per entry (GRLBWT_DEV_OVERLAP_EXPAND=f).  After a warm-up the variants take turns inside
each repetition; per variant the median, the fastest and the slowest.  Every call synchronises before it returns, so a host
clock around it is the call's time; an overlap call is two passes of its search, so its steps per second count each step once
for two executions.

Checked on the way: overlaps_of and overlaps write the same entries; the for_each form writes the same outputs as the tile
kernel; every read finds itself at L = 150 without PROPER.

Usage: python tools/gpu_fm_overlaps.py [--out profiles/fm_overlaps/overlaps.txt] [--reps 3] [--lib PATH] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIN_LEN = 50
COUNT_CELLS = 32


def set_env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def turns(variants, reps, say, what, unit):
    """variants: [(label, fn -> units of work)]; one warm-up each, then they take turns; -> {label: median seconds}"""
    work = {label: fn() for label, fn in variants}
    times = {label: [] for label, _ in variants}
    for _ in range(reps):
        for label, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[label].append(time.perf_counter() - t0)
    out = {}
    for label, _ in variants:
        ts = sorted(times[label])
        out[label] = statistics.median(ts)
        say("%-34s %-10s: median %9.3f ms  min %9.3f  max %9.3f  -> %6.2f G %s/s (%d)"
            % (what, label, out[label] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, work[label] / out[label] / 1e9, unit, work[label]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_overlaps", "overlaps.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="the development build: the tile kernel is also timed against the for_each form")
    ap.add_argument("--small", action="store_true", help="a tenth of the workload")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
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

    dev = args.lib is not None
    lib = args.lib or g.build_hip()
    n_reads, read_len, genome = (662251, 150, 3300000) if args.small else (6622517, 150, 33000000)
    say("grlbwt_fm_overlaps_of / grlbwt_fm_overlaps / grlbwt_fm_overlap_targets on %s (%s build)"
        % (torch.cuda.get_device_name(0), "development" if dev else "product"))
    text = workloads.sampled_reads_torch(n_reads, read_len, genome, device="cuda:0")
    torch.cuda.synchronize()
    Z = lambda n: torch.zeros(max(n, 1), dtype=torch.int64, device="cuda:0")
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()
        cells = text.view(n_reads, read_len + 1)[:, :read_len].contiguous()
        offsets = (torch.arange(n_reads + 1, dtype=torch.int64, device="cuda:0") * read_len).contiguous()
        ids = torch.arange(n_reads, dtype=torch.int64, device="cuda:0")
        t0 = time.perf_counter()
        with engine.FmIndex(ctx, image_ptr, nb, locate=True) as fm:
            info = fm.info()
            say("== %d reads of %d cells, %d cells, %d runs, image %d bytes; index with locate: %d bytes, idx_bytes %d, top_entries %d, made in %.0f ms"
                % (n_reads, read_len, text.numel(), runs, nb, info["index_bytes"], info["idx_bytes"], info["top_entries"], (time.perf_counter() - t0) * 1e3))
            assert info["n_strings"] == n_reads
            sizes = {}
            for fl in (0, engine.FM_OVERLAP_PROPER):
                try:
                    sizes[fl] = fm.overlaps_of(ids.data_ptr(), n_reads, MIN_LEN, 0, fl, None, None, None, None, 0)
                except engine.GrlbwtError as e:
                    sizes[fl] = e.n_hits
            cap = max(sizes.values())
            hoff = Z(n_reads + 1)
            cols = [Z(cap) for _ in range(3)]
            ref = {}

            def of(fl):
                fm.overlaps_of(ids.data_ptr(), n_reads, MIN_LEN, 0, fl, hoff.data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cap)
                return fm.overlap_info()["steps"]

            def by_cells(fl):
                fm.overlaps(cells.data_ptr(), 1, offsets.data_ptr(), n_reads, MIN_LEN, 0, fl, hoff.data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(),
                                cols[2].data_ptr(), cap)
                return fm.overlap_info()["steps"]

            def snapshot(n):
                return (hoff.clone(), cols[0][:n].clone(), cols[1][:n].clone(), cols[2][:n].clone())

            for fl, name in ((0, "all suffixes"), (engine.FM_OVERLAP_PROPER, "PROPER")):
                of(fl)
                i = fm.overlap_info()
                ref[fl] = snapshot(sizes[fl])
                say("min_len %d, %s: %d hits, %d targets, longest %d, cells %d, steps %d, lanes %d, refills %d"
                    % (MIN_LEN, name, i["n_hits"], i["n_targets"], i["longest"], i["n_cells"], i["steps"], i["walk_lanes"], i["lane_refills"]))
                if fl == 0:
                    last = ref[0][0][1:] - 1                       # every read's last hit: itself, at its whole length
                    assert bool((ref[0][1][last] == read_len).all()), "a read does not find itself at its whole length"
                by_cells(fl)
                assert all(torch.equal(a, b) for a, b in zip(ref[fl], snapshot(sizes[fl]))), "overlaps_of and overlaps disagree"
                variants = [("of", lambda fl=fl: of(fl)), ("cells", lambda fl=fl: by_cells(fl))]
                turns(variants, args.reps, say, "overlaps, %s" % name, "steps")
            # the targets of the first list, and one range of n_strings
            of(0)
            nh = sizes[0]
            nt = fm.overlap_info()["n_targets"]
            eoff, st, rg = Z(nh + 1), Z(nt), Z(nt)
            one_lo, one_hi = Z(1), torch.full((1,), n_reads, dtype=torch.int64, device="cuda:0")
            st1 = Z(n_reads)

            def tg(form=None):
                set_env("GRLBWT_DEV_OVERLAP_EXPAND", form)
                try:
                    return fm.overlap_targets(cols[1].data_ptr(), cols[2].data_ptr(), nh, eoff.data_ptr(), st.data_ptr(), nt, rg.data_ptr())
                finally:
                    set_env("GRLBWT_DEV_OVERLAP_EXPAND", None)

            def tg1(form=None):
                set_env("GRLBWT_DEV_OVERLAP_EXPAND", form)
                try:
                    return fm.overlap_targets(one_lo.data_ptr(), one_hi.data_ptr(), 1, eoff.data_ptr(), st1.data_ptr(), n_reads)
                finally:
                    set_env("GRLBWT_DEV_OVERLAP_EXPAND", None)

            assert tg() == nt
            say("targets: %d ranges, %d entries, tile_entries %d" % (nh, nt, fm.overlap_info()["tile_entries"]))
            v, v1 = [("tile", tg)], [("tile", tg1)]
            if dev:
                want = (st.clone(), rg.clone())
                tg("f")
                assert torch.equal(want[0], st) and torch.equal(want[1], rg), "the for_each form writes other entries"
                v.append(("for_each", lambda: tg("f")))
                v1.append(("for_each", lambda: tg1("f")))
            turns(v, args.reps, say, "targets of the hit list", "entries")
            turns(v1, args.reps, say, "targets, one range of n_strings", "entries")
            npat = min(1 << 20, cells.numel() // COUNT_CELLS)
            coff = (torch.arange(npat + 1, dtype=torch.int64, device="cuda:0") * COUNT_CELLS).contiguous()
            lo, hi = Z(npat), Z(npat)

            def count():
                fm.count(cells.data_ptr(), 1, coff.data_ptr(), npat, lo.data_ptr(), hi.data_ptr())
                return npat * COUNT_CELLS

            turns([("count", count)], args.reps, say, "grlbwt_fm_count, %d x %d cells" % (npat, COUNT_CELLS), "nominal steps")


if __name__ == "__main__":
    main()
