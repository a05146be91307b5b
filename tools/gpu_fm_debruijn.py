#!/usr/bin/env python3
"""grlbwt_debruijn_* on images of read collections at k = 21 and 31, with min_count 1 and 2: the create (nodes, edges, degrees,
unitigs) and the three writers.

ONE leg per invocation (--leg); the tool starts no child process.  Every leg is its own command under `timeout`, chained with `&&`:
    timeout -k 10 400 python tools/gpu_fm_debruijn.py --leg reads101 --lib tools/_build/libgrlbwt_dev.so --route-b &&
    timeout -k 10 900 python tools/gpu_fm_debruijn.py --leg reads1g --lib tools/_build/libgrlbwt_dev.so --route-b --append
Legs (grlbwt_amd/workloads.py, as tools/gpu_fm_kmers.py):
  reads101  1,000,000 x 100 bp uniform reads (101 MB)
  reads1g   6,622,517 x 150 bp reads sampled from a 33 Mbp genome (1 GB)

Per leg, k and min_count: the create timed `--reps` times; with a development library (--lib, built by tools/build_dev.sh) the tile
kernel of the unitigs' first cells and its generic form (GRLBWT_DEV_DEBRUIJN=f: a for_each over the nodes) take turns inside each
repetition and must give the same tables.  (The first run also compared a staged emit kernel of the edges under that switch; it
measured slower and was deleted; that run is kept as profiles/fm_debruijn/debruijn_staged_emit.txt.)  One more create of each form runs
under the library's profile: the kernels' times, grouped into the passes of the node selection, the edge count, the edge emit, the
unitigs (links, jumping rounds, placing) and the rest.  Then the writers, timed once per form: nodes + edges (copies) and the
unitigs with their cells.  Written: the graph's sizes, the create's median, the groups, backward steps per second of the two edge
passes, the cells' bytes per second.

--route-b: the route without these calls, timed once: grlbwt_fm_kmers for k and for k + 1 with their cells, both tables downloaded,
and joined on the host (numpy): the prefix and the suffix of every (k + 1)-mer looked up among the k-mers by a sort.  Its number
of edges must be n_edges (min_count 1 alone: the filter is applied to the nodes).

Usage: python tools/gpu_fm_debruijn.py --leg reads101|reads1g [--lib LIB] [--route-b] [--out profiles/fm_debruijn/debruijn.txt]
                                       [--append] [--reps 3] [--small]
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
GROUPS = (("node passes", ("lcp.", "kmer.")), ("edge count", ("debruijn.count",)), ("edge emit", ("debruijn.edges",)),
          ("unitigs", ("debruijn.links", "debruijn.heads", "debruijn.jump", "debruijn.open", "debruijn.cycle", "debruijn.unitig_ids",
                       "debruijn.circular", "debruijn.place", "debruijn.node_offsets", "debruijn.longest", "debruijn.order", "debruijn.weights")),
          ("first cells", ("debruijn.first_cells",)), ("tail cells", ("debruijn.tail_cells",)), ("rest", ("debruijn.",)))


def set_form(value):
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    if value is None:
        os.environ.pop("GRLBWT_DEV_DEBRUIJN", None)
    else:
        os.environ["GRLBWT_DEV_DEBRUIJN"] = value


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


def route_b(torch, np, fm, k, say):
    """the tables of k and k + 1, downloaded and joined on the host; returns the number of edges"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, a = fm.kmers(k, cell_bytes=1)
    _, cnt, b = fm.kmers(k + 1, cell_bytes=1)
    t1 = time.perf_counter()
    va = np.ascontiguousarray(a).view([("", a.dtype)] * k).reshape(-1)               # the k-mers, sorted as the table is
    pre = np.ascontiguousarray(b[:, :k]).view([("", b.dtype)] * k).reshape(-1)
    suf = np.ascontiguousarray(b[:, 1:]).view([("", b.dtype)] * k).reshape(-1)
    frm, to = np.searchsorted(va, pre), np.searchsorted(va, suf)
    order = np.lexsort((frm, to))
    edges = len(order)
    t2 = time.perf_counter()
    say("  route without the calls: the tables of k and k + 1 with their cells %.1f ms (%d and %d entries), the join on the host %.1f ms: %.1f ms, %d edges"
        % ((t1 - t0) * 1e3, len(a), len(b), (t2 - t1) * 1e3, (t2 - t0) * 1e3, edges))
    return edges


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
            say("== %s: %d cells, %d strings, %d runs, idx_bytes %d" % (name, info["n_syms"], info["n_strings"], runs, info["idx_bytes"]))
            for k in KS:
                for min_count in (1, 2):
                    def create(form):
                        set_form(form)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        h = fm.de_bruijn(k, min_count)
                        torch.cuda.synchronize()
                        return h, time.perf_counter() - t0

                    def tables(h, form):
                        set_form(form)
                        i = h.info()
                        n, m, u, nc = i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_cells"]
                        z = lambda c, dt=torch.int64: torch.zeros(max(c, 1), dtype=dt, device="cuda:0")
                        nodes = [z(n), z(n), z(n, torch.int32), z(n, torch.int32), z(n), z(n)]
                        edges = [z(n + 1), z(m), z(m), z(m)]
                        un = [z(u + 1), z(n), z(nc, torch.uint8), z(u), z(u, torch.uint8)]
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        h.nodes_raw(*[t.data_ptr() for t in nodes], capacity=n)
                        h.edges_raw(*[t.data_ptr() for t in edges], capacity=m)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        h.unitigs_raw(fm, 1, *[t.data_ptr() for t in un], capacity_unitigs=u, capacity_nodes=n, capacity_cells=nc)
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        return nodes + edges + un, t1 - t0, t2 - t1

                    ref, times = None, {label: [] for label, _ in forms}
                    for label, form in forms:                # warm-up, and both forms give the same tables
                        h, _ = create(form)
                        got, _, _ = tables(h, form)
                        h.close()
                        if ref is None:
                            ref = got
                        assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
                    del got
                    for _ in range(args.reps):
                        for label, form in forms:
                            h, t = create(form)
                            h.close()
                            times[label].append(t)
                    for label, form in forms:
                        ctx.profile_enable(True)
                        h, _ = create(form)
                        gr = grouped(ctx.profile())
                        ctx.profile_enable(False)
                        i = h.info()
                        if label == forms[0][0]:
                            say("k = %d, min_count = %d: %d nodes of %d distinct k-mers, %d edges (max in %d, out %d), %d unitigs (%d circular, longest %d nodes), "
                                "%d cells; %d + %d passes, %d jumping rounds; handle %d bytes, scratch %d bytes"
                                % (k, min_count, i["n_nodes"], i["n_distinct"], i["n_edges"], i["max_in_degree"], i["max_out_degree"], i["n_unitigs"],
                                   i["n_circular"], i["longest_unitig"], i["n_cells"], i["passes"], i["length_passes"], i["jump_rounds"], i["handle_bytes"],
                                   i["scratch_bytes"]))
                        ctx.profile_enable(True)
                        _, t_copy, t_cells = tables(h, form)
                        gw = grouped(ctx.profile())
                        ctx.profile_enable(False)
                        h.close()
                        ts = sorted(times[label])
                        ed = (gr["edge count"] + gr["edge emit"]) / 1e3
                        cl = (gw["first cells"] + gw["tail cells"]) / 1e3
                        say("  %-7s: create median %9.2f ms  min %9.2f  max %9.2f | kernels: node passes %8.2f, edge count %7.2f, edge emit %7.2f, unitigs %7.2f, "
                            "rest %6.2f ms -> %6.2f G backward steps/s | nodes + edges %7.2f ms, unitigs with cells %7.2f ms (first cells %6.3f, tail "
                            "cells %6.3f ms: %6.1f GB/s)"
                            % (label, statistics.median(ts) * 1e3, ts[0] * 1e3, ts[-1] * 1e3, gr["node passes"], gr["edge count"], gr["edge emit"],
                               gr["unitigs"], gr["rest"], i["backward_steps"] / ed / 1e9 if ed > 0 else 0.0, t_copy * 1e3, t_cells * 1e3,
                               gw["first cells"], gw["tail cells"], i["n_cells"] / cl / 1e9 if cl > 0 else 0.0))
                    set_form(None)
                    del ref
                    if args.route_b and min_count == 1:
                        assert route_b(torch, np, fm, k, say) == i["n_edges"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--lib", default=None, help="a development library (tools/build_dev.sh): the generic forms are measured too")
    ap.add_argument("--route-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_debruijn", "debruijn.txt"))
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
        say("grlbwt_debruijn_*: create and the writers, the tile kernel of the first cells (default) against the generic form (GRLBWT_DEV_DEBRUIJN=f) on %s%s"
            % (torch.cuda.get_device_name(0), "; collections cut to a sixteenth (--small)" if args.small else ""))
    measure(args.leg, args, say)


if __name__ == "__main__":
    main()
