#!/usr/bin/env python3
"""grlbwt_fm_approx on images of read collections: its two forms against each other -- lanes that take tickets
(prim::top_tickets, GRLBWT_FM_MATCH unset) and one lane per pattern (GRLBWT_FM_MATCH=l, prim::top_search) -- and against
grlbwt_fm_count on the same queries.

One process, no children.  Every step that uses the GPU runs under a time limit of its own (a timer that ends the process with
status 124 when the step has not returned), and the first failure ends the script.  For the 101 MB (1,000,000 x 100 bp uniform
reads) and the 1 GB (6,622,517 x 150 bp reads sampled from a 33 Mbp genome) workloads of grlbwt_amd/workloads.py: build the
image, make one index, and time grlbwt_fm_approx for 2^17 seeded queries of the read length -- a third whole reads cut from the
text, a third with one cell changed, a third with two -- at k = 0, 1, 2, and at k = 3 on 2^14 of them, each with max_hits 0 and
8.  After a warm-up the two forms take turns inside each repetition; per form the median, the fastest and the slowest of the
repetitions, the backward steps of the emitting pass and the steps per second over BOTH passes (2 x steps / time), the hits and
the lane refills.  The sizing call (capacity 0, no arrays) is the count pass alone: its median over the call's is the count
pass's share.  grlbwt_fm_count on the same queries is timed beside them: k = 0 takes two passes of the same steps, so its time
is to be read against twice the count's.  Nothing about the rate is fixed in advance.

Checked on the way: both forms write the same entries; at k >= the changes made, every query has a hit; a thousand sampled hits
of the k = 2 run: the variant rebuilt from sub_pos / sub_val counts to the same rows, and one row of it, located and extracted
from the index, reads back as that variant.

Usage: python tools/gpu_fm_approx.py [--out profiles/fm_approx/approx.txt] [--reps 9] [--queries 131072] [--small]
"""
import argparse
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = (("tickets", None), ("lanes", "l"))
MAX_HITS = (0, 8)


class Limit:
    """a time limit for one step: the process ends with status 124 when the step has not returned by then"""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def expire(self):
        print("TIME LIMIT of %d s: %s" % (self.seconds, self.what), flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self.expire)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *a):
        self.timer.cancel()


def set_form(value):
    if value is None:
        os.environ.pop("GRLBWT_FM_MATCH", None)
    else:
        os.environ["GRLBWT_FM_MATCH"] = value


def queries_from(torch, text, n_reads, read_len, n_q, seed):
    """n_q x read_len cells: whole reads; the second third with one cell rotated within ACGT, the last third with two"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = text.device
    reads = torch.randint(0, n_reads, (n_q,), generator=g).to(dev)
    span = torch.arange(read_len, device=dev)[None, :]
    cells = text[(reads * (read_len + 1))[:, None] + span].clone()
    third = n_q // 3
    rot = torch.zeros(256, dtype=torch.uint8, device=dev)
    rot[torch.tensor([65, 67, 71, 84], device=dev)] = torch.tensor([67, 71, 84, 65], dtype=torch.uint8, device=dev)
    for first, n_changes in ((third, 1), (2 * third, 2)):
        rows = torch.arange(first, n_q if n_changes == 2 else 2 * third, device=dev)
        where = torch.randperm(read_len, generator=g)[:2].to(dev)           # two different offsets, rotated by a shift of the query's own
        shift = torch.randint(0, read_len, (len(rows),), generator=g).to(dev)
        for c in range(n_changes):
            at = (where[c] + shift) % read_len
            cells[rows, at] = rot[cells[rows, at].long()]
    return cells.contiguous(), third


class Buffers:
    def __init__(self, torch, nq, cap, k):
        z = lambda n: torch.zeros(max(n, 1), dtype=torch.int64, device="cuda:0")
        self.cap, self.k = cap, k
        self.hoff, self.mism, self.lo, self.hi, self.sp, self.sv = z(nq + 1), z(cap), z(cap), z(cap), z(cap * k), z(cap * k)

    def snapshot(self, n):
        return [t[:m].clone() for t, m in ((self.hoff, len(self.hoff)), (self.mism, n), (self.lo, n), (self.hi, n), (self.sp, n * self.k), (self.sv, n * self.k))]


def measure(name, make_text, n_reads, read_len, args, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine
    lib = g.build_hip()
    with Limit(120, name + ": the text"):
        text = make_text()
        torch.cuda.synchronize()
    nq = args.queries
    out = {}
    with engine.Context(0, 0, lib) as ctx:
        with Limit(600, name + ": the build"):
            ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
            ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        with Limit(120, name + ": the queries"):
            cells, third = queries_from(torch, text, n_reads, read_len, nq, 20261019)
            offsets = (torch.arange(nq + 1, dtype=torch.int64, device="cuda:0") * read_len).contiguous()
            torch.cuda.synchronize()
        say("== %s: %d cells, %d runs, image %d bytes; %d queries of %d cells (%d cut, %d with one cell changed, %d with two)"
            % (name, text.numel(), runs, nb, nq, read_len, third, third, nq - 2 * third))
        set_form(None)
        with Limit(300, name + ": the index"):
            fm = engine.FmIndex(ctx, image_ptr, nb)
        with fm:
            info = fm.info()
            say("index: %d bytes, idx_bytes %d, top_entries %d, sigma %d" % (info["index_bytes"], info["idx_bytes"], info["top_entries"], info["sigma"]))
            # grlbwt_fm_count on the same queries
            clo = torch.zeros(nq, dtype=torch.int64, device="cuda:0")
            chi = torch.zeros(nq, dtype=torch.int64, device="cuda:0")
            ts = []
            with Limit(120, name + ": count"):
                for r in range(args.reps + 2):
                    t0 = time.perf_counter()
                    fm.count(cells.data_ptr(), 1, offsets.data_ptr(), nq, clo.data_ptr(), chi.data_ptr())
                    if r >= 2:
                        ts.append(time.perf_counter() - t0)
            ts.sort()
            count_med = statistics.median(ts)
            found = int((chi > clo).sum())
            say("grlbwt_fm_count, the %d queries whole: median %8.3f ms  min %8.3f  max %8.3f (%d found; a query that is not found ends early)"
                % (nq, count_med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, found))
            for k in (0, 1, 2, 3):
                n = nq if k < 3 else min(nq, 1 << 14)
                sel = torch.arange(0, nq, nq // n, device="cuda:0")[:n] if n < nq else None
                qc = cells if sel is None else cells[sel].contiguous()
                for mh in MAX_HITS:
                    label = "k %d max_hits %d" % (k, mh)

                    def sizing(form):
                        set_form(form)
                        t0 = time.perf_counter()
                        try:
                            got = fm.approx(qc.data_ptr(), 1, offsets.data_ptr(), n, k, mh, None, None, None, None, 0)
                        except engine.GrlbwtError as e:
                            assert e.code == -22, e
                            got = e.n_hits
                        return time.perf_counter() - t0, got

                    with Limit(300, "%s: %s, sizing" % (name, label)):
                        _, cap = sizing(None)
                    B = Buffers(torch, n, cap, k)

                    def call(form):
                        set_form(form)
                        t0 = time.perf_counter()
                        got = fm.approx(qc.data_ptr(), 1, offsets.data_ptr(), n, k, mh, B.hoff.data_ptr(), B.mism.data_ptr(), B.lo.data_ptr(),
                                        B.hi.data_ptr(), cap, B.sp.data_ptr() if k else None, B.sv.data_ptr() if k else None)
                        assert got == cap, (got, cap)
                        return time.perf_counter() - t0

                    ref, infos = None, {}
                    for form_label, form in FORMS:           # warm-up, and both forms write the same
                        with Limit(300, "%s: %s, %s, warm-up" % (name, label, form_label)):
                            call(form)
                            call(form)
                            infos[form_label] = fm.approx_info()
                            got = B.snapshot(cap)
                        if ref is None:
                            ref = got
                        assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
                    per = ref[0][1:] - ref[0][:-1]
                    rows = torch.arange(n, device="cuda:0") if sel is None else sel
                    changes = (rows >= third).long() + (rows >= 2 * third).long()
                    assert bool((per[changes <= k] >= 1).all()), "a query with no more changes than k has no hit"
                    times = {fl: [] for fl, _ in FORMS}
                    sizes = []
                    with Limit(600, "%s: %s, the repetitions" % (name, label)):
                        for _ in range(args.reps):
                            for form_label, form in FORMS:
                                times[form_label].append(call(form))
                            sizes.append(sizing(None)[0])
                    set_form(None)
                    for form_label, _ in FORMS:
                        ts = sorted(times[form_label])
                        med = statistics.median(ts)
                        i = infos[form_label]
                        out[(form_label, k, mh)] = (med, ts[0], ts[-1])
                        say("%s %-7s: median %9.3f ms  min %9.3f  max %9.3f  -> %6.2f G steps/s over both passes (%d steps in the emitting pass), %d hits "
                            "%s, %d cut, lanes %d, refills %d" % (label, form_label, med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, 2 * i["steps"] / med / 1e9, i["steps"],
                                                                 i["n_hits"], i["hits_by_mismatches"][:k + 1], i["n_truncated"], i["walk_lanes"], i["lane_refills"]))
                    smed = statistics.median(sizes)
                    say("%s sizing : median %9.3f ms: the count pass is %.0f %% of the tickets call%s"
                        % (label, smed * 1e3, 100 * smed / out[("tickets", k, mh)][0],
                           "; twice grlbwt_fm_count is %.3f ms" % (2e3 * count_med * n / nq) if k == 0 else ""))
                    if k == 2 and mh == 0:
                        keep = (qc, ref, cap)
        # a thousand hits of the k = 2 run: the rebuilt variant counts to the same rows, and reads back from the index
        with Limit(600, name + ": the index that locates and extracts"):
            fm = engine.FmIndex(ctx, image_ptr, nb, locate=True, extract=True)
        with fm, Limit(300, name + ": the thousand hits"):
            qc, ref, cap = keep
            hoff, mism, lo, hi, sp, sv = ref
            pick = torch.arange(0, cap, max(cap // 1000, 1), device="cuda:0")[:1000]
            m = len(pick)
            pat = torch.searchsorted(hoff[1:].contiguous(), pick, right=True)
            var = qc[pat].clone()
            P, V = sp.view(cap, 2)[pick], sv.view(cap, 2)[pick]
            for t in range(2):
                use = P[:, t] >= 0                               # (UINT64_MAX reads as -1)
                assert bool((use == (mism[pick] > t)).all())
                r = torch.arange(m, device="cuda:0")[use]
                assert bool((var[r, P[use, t]] != V[use, t].to(torch.uint8)).all()), "a substitute equals the pattern's cell"
                var[r, P[use, t]] = V[use, t].to(torch.uint8)
            var = var.contiguous()
            voff = (torch.arange(m + 1, dtype=torch.int64, device="cuda:0") * read_len).contiguous()
            vlo = torch.zeros(m, dtype=torch.int64, device="cuda:0")
            vhi = torch.zeros(m, dtype=torch.int64, device="cuda:0")
            fm.count(var.data_ptr(), 1, voff.data_ptr(), m, vlo.data_ptr(), vhi.data_ptr())
            assert torch.equal(vlo, lo[pick]) and torch.equal(vhi, hi[pick]), "a rebuilt variant does not count to the hit's rows"
            s = torch.zeros(m, dtype=torch.int64, device="cuda:0")
            o = torch.zeros(m, dtype=torch.int64, device="cuda:0")
            fm.locate(vlo.data_ptr(), m, engine.UINT64_MAX, s.data_ptr(), o.data_ptr())
            end = (o + read_len).contiguous()
            back = torch.zeros(m * read_len, dtype=torch.uint8, device="cuda:0")
            boff = torch.zeros(m + 1, dtype=torch.int64, device="cuda:0")
            got = fm.extract(s.data_ptr(), o.data_ptr(), end.data_ptr(), m, 1, back.data_ptr(), m * read_len, boff.data_ptr())
            assert got == m * read_len and torch.equal(back.view(m, read_len), var), "a located hit does not read as its variant"
            say("hits: %d of the %d of k 2 rebuilt from sub_pos / sub_val: each counts to its rows; located and extracted (%d cells), each reads as its variant"
                % (m, cap, got))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_approx", "approx.txt"))
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

    say("grlbwt_fm_approx as tickets (default) and as lanes (GRLBWT_FM_MATCH=l) on %s" % torch.cuda.get_device_name(0))
    res = {"101MB": measure("101 MB uniform reads", lambda: workloads.uniform_reads_torch(1000000, 100, device="cuda:0"), 1000000, 100, args, say)}
    if not args.small:
        res["1GB"] = measure("1 GB sampled reads", lambda: workloads.sampled_reads_torch(6622517, 150, 33000000, device="cuda:0"), 6622517, 150, args, say)
    for k in (0, 1, 2, 3):
        for mh in MAX_HITS:
            for name, med in res.items():
                t, l = med[("tickets", k, mh)], med[("lanes", k, mh)]
                spread = max(t[2] - t[1], l[2] - l[1])
                verdict = "tickets" if t[0] < l[0] - spread else "lanes" if l[0] < t[0] - spread else "within the spread"
                say("%s, k %d max_hits %d: tickets %.3f ms, lanes %.3f ms, spread of the repetitions %.3f ms: %s"
                    % (name, k, mh, t[0] * 1e3, l[0] * 1e3, spread * 1e3, verdict))


if __name__ == "__main__":
    main()
