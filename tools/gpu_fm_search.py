#!/usr/bin/env python3
"""What the LDS top level of the FM index's searches is worth (GRLBWT_FM_TOP_BITS), on images of read collections.

One process, no children.  For the 101 MB (1,000,000 x 100 bp uniform reads) and the 1 GB (6,622,517 x 150 bp reads sampled
from a 33 Mbp genome) workloads of grlbwt_amd/workloads.py: build the image, make one index per setting (0, 8, 12: the
switch is read when an index is made), and time grlbwt_fm_count for 2^20 patterns of 32 cells -- half of them cut from
the text, half of those with one cell changed.  After a warm-up the settings take turns, so that whatever else the
machine does falls on all of them alike; per setting the median, the fastest and the slowest of the repetitions.  The
call returns when the ranges are written (it synchronises), so a host clock around it is the call's time.

The cut patterns must all be found, and a thousand of their first rows are located and compared with the text.

Usage: python tools/gpu_fm_search.py [--out profiles/fm_index/count.txt] [--reps 9] [--patterns 1048576] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = (0, 8, 12)
CELLS = 32


def patterns_from(torch, text, n_reads, read_len, n_pat, seed):
    """n_pat x CELLS cells cut from reads at seeded places; the second half with one cell rotated within ACGT"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    reads = torch.randint(0, n_reads, (n_pat,), generator=g).to(text.device)
    offs = torch.randint(0, read_len - CELLS + 1, (n_pat,), generator=g).to(text.device)
    at = reads * (read_len + 1) + offs
    cells = text[at[:, None] + torch.arange(CELLS, device=text.device)[None, :]].clone()
    where = torch.randint(0, CELLS, (n_pat,), generator=g).to(text.device)
    half = n_pat // 2
    rows = torch.arange(half, n_pat, device=text.device)
    rot = torch.zeros(256, dtype=torch.uint8, device=text.device)
    rot[torch.tensor([65, 67, 71, 84], device=text.device)] = torch.tensor([67, 71, 84, 65], dtype=torch.uint8, device=text.device)
    cells[rows, where[half:]] = rot[cells[rows, where[half:]].long()]
    return cells.contiguous(), reads, offs, half


def measure(name, make_text, n_reads, read_len, args, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine
    lib = g.build_hip()
    text = make_text()
    torch.cuda.synchronize()
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        t0 = time.perf_counter()
        ctx.build()
        t_build = time.perf_counter() - t0
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        cells, reads, offs, half = patterns_from(torch, text, n_reads, read_len, args.patterns, 20261018)
        offsets = (torch.arange(args.patterns + 1, dtype=torch.int64, device="cuda:0") * CELLS).contiguous()
        lo = torch.zeros(args.patterns, dtype=torch.int64, device="cuda:0")
        hi = torch.zeros(args.patterns, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        say("== %s: %d cells, %d runs, image %d bytes, engine build %.3f s" % (name, text.numel(), runs, nb, t_build))
        fms, t_make = {}, {}
        for b in SETTINGS:
            os.environ["GRLBWT_FM_TOP_BITS"] = str(b)
            t0 = time.perf_counter()
            fms[b] = engine.FmIndex(ctx, image_ptr, nb)
            t_make[b] = time.perf_counter() - t0
        del os.environ["GRLBWT_FM_TOP_BITS"]
        info = fms[SETTINGS[0]].info()
        say("index: %d bytes (%.2f per run), idx_bytes %d, sigma %d, strings %d; made in %s s (count only, first call warms the sorts)"
            % (info["index_bytes"], info["index_bytes"] / max(info["n_runs"], 1), info["idx_bytes"], info["sigma"], info["n_strings"],
               " / ".join("%.3f" % t_make[b] for b in SETTINGS)))

        def call(b):
            t0 = time.perf_counter()
            fms[b].count(cells.data_ptr(), 1, offsets.data_ptr(), args.patterns, lo.data_ptr(), hi.data_ptr())
            return time.perf_counter() - t0

        ref = None
        for b in SETTINGS:                               # warm-up, and every setting gives the same ranges
            call(b)
            call(b)
            got = (lo.clone(), hi.clone())
            assert bool((got[1][:half] > got[0][:half]).all()), "a pattern cut from the text was not found"
            if ref is None:
                ref = got
                found = int((got[1] > got[0]).sum())
            assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), "settings disagree"
        times = {b: [] for b in SETTINGS}
        for _ in range(args.reps):
            for b in SETTINGS:
                times[b].append(call(b))
        for b in SETTINGS:
            ts = sorted(times[b])
            med = statistics.median(ts)
            say("top_bits %2d (top_entries %4d): median %8.3f ms  min %8.3f  max %8.3f  -> %7.1f M patterns/s, %7.2f G nominal steps/s"
                % (b, fms[b].info()["top_entries"], med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, args.patterns / med / 1e6, args.patterns * CELLS / med / 1e9))
        say("patterns: %d of %d cells, %d found (the %d cut from the text and %d of the changed ones); %d repetitions, settings in turn"
            % (args.patterns, CELLS, found, half, found - half, args.reps))
        for fm in fms.values():
            fm.close()
        # a thousand first rows, located and compared with the text
        with engine.FmIndex(ctx, image_ptr, nb, locate=True) as fm:
            say("index with the locate structures: %d bytes" % fm.info()["index_bytes"])
            k = min(1000, half)
            rows = ref[0][:k].contiguous()
            s = torch.zeros(k, dtype=torch.int64, device="cuda:0")
            o = torch.zeros(k, dtype=torch.int64, device="cuda:0")
            t0 = time.perf_counter()
            fm.locate(rows.data_ptr(), k, engine.UINT64_MAX, s.data_ptr(), o.data_ptr())
            t_loc = time.perf_counter() - t0
            at = s * (read_len + 1) + o
            back = text[at[:, None] + torch.arange(CELLS, device="cuda:0")[None, :]]
            assert torch.equal(back, cells[:k]), "a located occurrence does not read as its pattern"
            say("locate: %d rows in %.3f ms, every occurrence reads as its pattern" % (k, t_loc * 1e3))
    medians = {b: statistics.median(times[b]) for b in SETTINGS}
    return medians


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_index", "count.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--patterns", type=int, default=1 << 20)
    ap.add_argument("--small", action="store_true", help="the 101 MB workload only")
    args = ap.parse_args()
    import torch
    from grlbwt_amd import workloads
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

    say("grlbwt_fm_count under GRLBWT_FM_TOP_BITS = %s on %s" % (", ".join(map(str, SETTINGS)), torch.cuda.get_device_name(0)))
    res = {"101MB": measure("101 MB uniform reads", lambda: workloads.uniform_reads_torch(1000000, 100, device="cuda:0"), 1000000, 100, args, say)}
    if not args.small:
        res["1GB"] = measure("1 GB sampled reads", lambda: workloads.sampled_reads_torch(6622517, 150, 33000000, device="cuda:0"), 6622517, 150, args, say)
    for name, med in res.items():
        best = min(med, key=med.get)
        say("%s: fastest median at top_bits %d (%s)" % (name, best, ", ".join("%d: %.3f ms" % (b, med[b] * 1e3) for b in SETTINGS)))


if __name__ == "__main__":
    main()
