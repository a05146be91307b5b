#!/usr/bin/env python3
"""The two forms of grlbwt_fm_match against each other -- lanes that take tickets (prim::top_tickets, GRLBWT_FM_MATCH unset)
and one lane per query cell (GRLBWT_FM_MATCH=l, prim::top_search) -- on images of read collections.

One process, no children.  For the 101 MB (1,000,000 x 100 bp uniform reads) and the 1 GB (6,622,517 x 150 bp reads sampled
from a 33 Mbp genome) workloads of grlbwt_amd/workloads.py: build the image, make one index, and time grlbwt_fm_match for 2^17
queries of the read length -- a third whole reads cut from the text, a third of those with two cells changed, a third
chimeras of the halves of two reads -- with max_len 32 and 0.  After a warm-up the two forms take turns inside each
repetition, so that whatever else the machine does falls on both alike; per form the median, the fastest and the slowest of
the repetitions, and the steps per second from matched_cells + n_cells.  The call returns when the lengths are written (it
synchronises), so a host clock around it is the call's time.  grlbwt_fm_count on 2^20 patterns of 32 cells is timed beside
them as the reference for one step's cost (profiles/fm_index/count.txt): context, not a pass mark.

Checked on the way: both forms write the same lengths and rows; every cut query reports its full length (or the cap) at its
last end; one row of each of a thousand reported MEMs is located, the text there extracted from the index and compared with
the query's piece.

Usage: python tools/gpu_fm_match.py [--out profiles/fm_match/match.txt] [--reps 9] [--queries 131072] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = (("tickets", None), ("lanes", "l"))
CAPS = (32, 0)
COUNT_CELLS = 32


def set_form(value):
    if value is None:
        os.environ.pop("GRLBWT_FM_MATCH", None)
    else:
        os.environ["GRLBWT_FM_MATCH"] = value


def queries_from(torch, text, n_reads, read_len, n_q, seed):
    """n_q x read_len cells: whole reads; the second third with two cells rotated within ACGT; the last third the first half of
    one read in front of the second half of another"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = text.device
    reads = torch.randint(0, n_reads, (n_q,), generator=g).to(dev)
    other = torch.randint(0, n_reads, (n_q,), generator=g).to(dev)
    span = torch.arange(read_len, device=dev)[None, :]
    cells = text[(reads * (read_len + 1))[:, None] + span].clone()
    third = n_q // 3
    rot = torch.zeros(256, dtype=torch.uint8, device=dev)
    rot[torch.tensor([65, 67, 71, 84], device=dev)] = torch.tensor([67, 71, 84, 65], dtype=torch.uint8, device=dev)
    rows = torch.arange(third, 2 * third, device=dev)
    for _ in range(2):
        where = torch.randint(0, read_len, (third,), generator=g).to(dev)
        cells[rows, where] = rot[cells[rows, where].long()]
    half = read_len // 2
    cells[2 * third:, half:] = text[(other[2 * third:] * (read_len + 1))[:, None] + span][:, half:]
    return cells.contiguous(), third


def measure(name, make_text, n_reads, read_len, args, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine
    lib = g.build_hip()
    text = make_text()
    torch.cuda.synchronize()
    nq = args.queries
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        cells, third = queries_from(torch, text, n_reads, read_len, nq, 20261019)
        nc = nq * read_len
        offsets = (torch.arange(nq + 1, dtype=torch.int64, device="cuda:0") * read_len).contiguous()
        L = torch.zeros(nc, dtype=torch.int64, device="cuda:0")
        lo = torch.zeros(nc, dtype=torch.int64, device="cuda:0")
        hi = torch.zeros(nc, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        say("== %s: %d cells, %d runs, image %d bytes; %d queries of %d cells (%d cut, %d with two cells changed, %d chimeras)"
            % (name, text.numel(), runs, nb, nq, read_len, third, third, nq - 2 * third))
        set_form(None)
        medians = {}
        with engine.FmIndex(ctx, image_ptr, nb) as fm:
            info = fm.info()
            say("index: %d bytes, idx_bytes %d, top_entries %d" % (info["index_bytes"], info["idx_bytes"], info["top_entries"]))

            def call(form, cap):
                set_form(form)
                t0 = time.perf_counter()
                fm.match(cells.data_ptr(), 1, offsets.data_ptr(), nq, cap, L.data_ptr(), lo.data_ptr(), hi.data_ptr())
                return time.perf_counter() - t0

            for cap in CAPS:
                ref, infos = None, {}
                for label, form in FORMS:                # warm-up, and both forms write the same
                    call(form, cap)
                    call(form, cap)
                    infos[label] = fm.match_info()
                    got = (L.clone(), lo.clone(), hi.clone())
                    last = got[0].view(nq, read_len)[:third, -1]
                    assert bool((last == (min(cap, read_len) if cap else read_len)).all()), "a cut query does not match whole at its last end"
                    if ref is None:
                        ref = got
                    assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
                times = {label: [] for label, _ in FORMS}
                for _ in range(args.reps):
                    for label, form in FORMS:
                        times[label].append(call(form, cap))
                for label, _ in FORMS:
                    ts = sorted(times[label])
                    med = statistics.median(ts)
                    i = infos[label]
                    steps = i["matched_cells"] + i["n_cells"]
                    medians[(label, cap)] = (med, ts[0], ts[-1])
                    say("max_len %2d %-7s: median %8.3f ms  min %8.3f  max %8.3f  -> %6.2f G steps/s (%d steps: matched %d + cells %d; longest %d, "
                        "capped %d), lanes %d, refills %d" % (cap, label, med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, steps / med / 1e9, steps, i["matched_cells"],
                                                             i["n_cells"], i["longest"], i["n_capped"], i["walk_lanes"], i["lane_refills"]))
            set_form(None)
            # the parent's count on the same box: 2^20 patterns of 32 cells, the first half of every query
            npat = min(1 << 20, nc // COUNT_CELLS)
            coff = (torch.arange(npat + 1, dtype=torch.int64, device="cuda:0") * COUNT_CELLS).contiguous()
            ts = []
            for r in range(args.reps + 2):
                t0 = time.perf_counter()
                fm.count(cells.data_ptr(), 1, coff.data_ptr(), npat, lo.data_ptr(), hi.data_ptr())
                if r >= 2:
                    ts.append(time.perf_counter() - t0)
            ts.sort()
            med = statistics.median(ts)
            say("grlbwt_fm_count, %d patterns of %d cells (consecutive pieces of the queries): median %8.3f ms  min %8.3f  max %8.3f  -> %6.2f G nominal steps/s"
                % (npat, COUNT_CELLS, med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, npat * COUNT_CELLS / med / 1e9))
        # a thousand MEMs of 20 cells and more: one row each located, the text there extracted and compared
        with engine.FmIndex(ctx, image_ptr, nb, locate=True, extract=True) as fm:
            sub = torch.arange(0, nq, max(nq // 1500, 1), device="cuda:0")[:1500]
            qs = cells[sub].contiguous()
            k = len(sub)
            qoff = (torch.arange(k + 1, dtype=torch.int64, device="cuda:0") * read_len).contiguous()
            cap_m = k * read_len
            out = [torch.zeros(cap_m, dtype=torch.int64, device="cuda:0") for _ in range(5)]
            n = fm.mems(qs.data_ptr(), 1, qoff.data_ptr(), k, 20, 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cap_m,
                        out[3].data_ptr(), out[4].data_ptr())
            assert n >= 1000, n
            pick = torch.arange(0, n, n // 1000, device="cuda:0")[:1000]
            pat, beg, mlen, mlo, mhi = (o[:n][pick].contiguous() for o in out)
            assert bool((mhi > mlo).all())
            s = torch.zeros(1000, dtype=torch.int64, device="cuda:0")
            o = torch.zeros(1000, dtype=torch.int64, device="cuda:0")
            fm.locate(mlo.data_ptr(), 1000, engine.UINT64_MAX, s.data_ptr(), o.data_ptr())
            end = (o + mlen).contiguous()
            total = int(mlen.sum())
            back = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
            boff = torch.zeros(1001, dtype=torch.int64, device="cuda:0")
            got = fm.extract(s.data_ptr(), o.data_ptr(), end.data_ptr(), 1000, 1, back.data_ptr(), total, boff.data_ptr())
            assert got == total
            want = torch.cat([qs[int(p), int(b):int(b) + int(m)] for p, b, m in zip(pat.tolist(), beg.tolist(), mlen.tolist())])
            assert torch.equal(back, want), "a located MEM does not read as its piece of the query"
            say("mems: %d of 20 cells and more in %d queries; 1000 of them located and extracted (%d cells), every one reads as its piece of the query"
                % (n, k, total))
    return medians


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_match", "match.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--queries", type=int, default=1 << 17)
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

    say("grlbwt_fm_match as tickets (default) and as lanes (GRLBWT_FM_MATCH=l) on %s" % torch.cuda.get_device_name(0))
    res = {"101MB": measure("101 MB uniform reads", lambda: workloads.uniform_reads_torch(1000000, 100, device="cuda:0"), 1000000, 100, args, say)}
    if not args.small:
        res["1GB"] = measure("1 GB sampled reads", lambda: workloads.sampled_reads_torch(6622517, 150, 33000000, device="cuda:0"), 6622517, 150, args, say)
    for cap in CAPS:
        verdicts = []
        for name, med in res.items():
            t, l = med[("tickets", cap)], med[("lanes", cap)]
            spread = max(t[2] - t[1], l[2] - l[1])
            verdicts.append("tickets" if t[0] < l[0] - spread else "lanes" if l[0] < t[0] - spread else "within the spread")
            say("%s, max_len %d: tickets %.3f ms, lanes %.3f ms, spread of the repetitions %.3f ms: %s"
                % (name, cap, t[0] * 1e3, l[0] * 1e3, spread * 1e3, verdicts[-1]))


if __name__ == "__main__":
    main()
