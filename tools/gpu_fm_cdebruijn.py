#!/usr/bin/env python3
"""grlbwt_cdebruijn_* on images of read collections at k = 31, each collection as it is (one strand) and with the reverse
complement of every read behind it (both strands, what -R writes): the create, split into its passes, and the three writers.

ONE leg per invocation (--leg); the tool starts no child process.  Every leg is its own command under `timeout`, chained with `&&`:
    timeout -k 10 300 python tools/gpu_fm_cdebruijn.py --leg reads101 --lib tools/_build/libgrlbwt_dev.so --route-b &&
    timeout -k 10 300 python tools/gpu_fm_cdebruijn.py --leg reads101x2 --lib tools/_build/libgrlbwt_dev.so --route-b --append
Legs (grlbwt_amd/workloads.py, as tools/gpu_fm_debruijn.py); x2: both strands
  reads101, reads101x2  1,000,000 x 100 bp uniform reads (101 MB)
  reads1g, reads1gx2    6,622,517 x 150 bp reads sampled from a 33 Mbp genome (1 GB)

Per leg: the create timed `--reps` times; with a development library (--lib, built by tools/build_dev.sh) the new kernels -- the
fused merge, the tile kernel of the first cells with the walks as tickets -- and their generic forms (GRLBWT_DEV_CDEBRUIJN=f) take
turns inside each repetition and must give the same tables.  One more create of each form runs under the library's profile: the
kernels' times, grouped into the node passes, the mate pass, the edge search, the merge (keys, sorts, flags, entries, offsets)
and the unitigs.  Then the writers, timed once per form: nodes + links (copies) and the unitigs with their cells.

--route-b: the route without the call, timed once: de_bruijn(k) and canonical_kmers(k) without cells, the nodes, the edges and the
class table downloaded, the ends and the merged half-edge table made on the host (numpy).  Its number of half-edges must be
n_half_edges.

Usage: python tools/gpu_fm_cdebruijn.py --leg LEG [--lib LIB] [--route-b] [--out profiles/fm_cdebruijn/cdebruijn.txt] [--append]
                                        [--reps 3] [--small] [--k 31]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("reads101", "reads101x2", "reads1g", "reads1gx2")
GROUPS = (("mate pass", ("ckmer.mates",)), ("node passes", ("lcp.", "kmer.", "ckmer.", "cdebruijn.nodes", "cdebruijn.rigid", "cdebruijn.palindromes",
                                                            "cdebruijn.heads", "cdebruijn.head_", "debruijn.fingerprint")),
          ("edge search", ("cdebruijn.count", "cdebruijn.records", "cdebruijn.record_offsets", "cdebruijn.steps")),
          ("merge kernels", ("cdebruijn.flags", "cdebruijn.tile_offsets", "cdebruijn.merge", "cdebruijn.groups", "cdebruijn.group_ranks")),
          ("merge rest", ("cdebruijn.keys", "cdebruijn.sort", "cdebruijn.hairpins", "cdebruijn.end_offsets", "cdebruijn.self", "cdebruijn.max_degree")),
          ("first cells", ("cdebruijn.first_cells", "cdebruijn.walk")), ("tail cells", ("cdebruijn.tail_cells",)),
          ("copies", ("cdebruijn.copy",)), ("unitigs", ("cdebruijn.",)), ("rest", ("",)))


def set_form(value):
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    if value is None:
        os.environ.pop("GRLBWT_DEV_CDEBRUIJN", None)
    else:
        os.environ["GRLBWT_DEV_CDEBRUIJN"] = value


def make_text(torch, workloads, leg, small):
    div = 16 if small else 1
    if leg.startswith("reads101"):
        name, L, text = "101 MB uniform reads", 100, workloads.uniform_reads_torch(1000000 // div, 100, device="cuda:0")
    else:
        name, L, text = "1 GB sampled reads", 150, workloads.sampled_reads_torch(6622517 // div, 150, 33000000 // div, device="cuda:0")
    if not leg.endswith("x2"):
        return name + ", one strand", text
    comp = torch.arange(256, dtype=torch.uint8, device="cuda:0")
    for a, b in ((65, 84), (67, 71)):
        comp[a], comp[b] = b, a
    rows = text.view(-1, L + 1)
    rc = rows.clone()
    rc[:, :L] = comp[torch.flip(rows[:, :L], dims=(1,)).long()]
    return name + ", both strands", torch.cat([text, rc.reshape(-1)])


def grouped(prof):
    out = {g: 0.0 for g, _ in GROUPS}
    for name, (_, ms, _) in prof.items():
        for g, prefixes in GROUPS:
            if any(name.startswith(p) for p in prefixes):
                out[g] += ms
                break
    return out


def route_b(torch, np, fm, k, say):
    """the plain graph and the class table, downloaded and merged on the host; returns the number of half-edges"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with fm.de_bruijn(k) as g:
        plo = g.nodes()["lo"]
        off, frm, wt, _ = g.edges()
    clo, _, mate, _, _ = fm.canonical_kmers(k, cells=False)
    t1 = time.perf_counter()
    none = np.uint64(2 ** 64 - 1)
    node = np.searchsorted(clo, plo)                          # a representative's own class ...
    node[node >= len(clo)] = 0
    is_rep = clo[node] == plo
    has = np.flatnonzero((mate != none) & (mate != clo))
    order = has[np.argsort(mate[has], kind="stable")]
    at = np.searchsorted(mate[order], plo[~is_rep])
    node[~is_rep] = order[at]                                 # ... a mate's through the sorted mate_lo
    pal = (mate == clo)[node] & is_rep
    to = np.repeat(np.arange(len(plo)), np.diff(off.astype(np.int64)))
    f = frm.astype(np.int64)
    a = 2 * node[f] + np.where(is_rep[f] & ~pal[f], 1, 0)
    b = 2 * node[to] + np.where(is_rep[to], 0, 1)
    keep = a != b
    src, oth, w = np.concatenate([a, b[keep]]), np.concatenate([b, a[keep]]), np.concatenate([wt, wt[keep]])
    o = np.lexsort((oth, src))
    src, oth, w = src[o], oth[o], w[o]
    head = np.concatenate([[True], (src[1:] != src[:-1]) | (oth[1:] != oth[:-1])]) if len(src) else np.zeros(0, dtype=bool)
    merged = np.add.reduceat(w, np.flatnonzero(head)) if len(src) else w
    ends = np.searchsorted(src[head], np.arange(2 * len(clo) + 1))
    t2 = time.perf_counter()
    say("  route without the call: de_bruijn + canonical_kmers with their downloads %.1f ms (%d nodes, %d edges, %d classes), the ends and the merge on "
        "the host %.1f ms: %.1f ms, %d half-edges" % ((t1 - t0) * 1e3, len(plo), len(frm), len(clo), (t2 - t1) * 1e3, (t2 - t0) * 1e3, len(merged)))
    assert int(ends[-1]) == len(merged)
    return len(merged)


def measure(leg, args, say):
    import numpy as np
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
    lib = os.path.abspath(args.lib) if args.lib else g.build_hip()
    forms = (("kernels", None), ("generic", "f")) if args.lib else (("kernels", None),)
    name, text = make_text(torch, workloads, leg, args.small)
    k = args.k
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

            def create(form):
                set_form(form)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = fm.de_bruijn_canonical(k)
                torch.cuda.synchronize()
                return h, time.perf_counter() - t0

            def tables(h, form):
                set_form(form)
                i = h.info()
                n, m, u, nc = i["n_nodes"], i["n_half_edges"], i["n_unitigs"], i["n_cells"]
                z = lambda c, dt=torch.int64: torch.zeros(max(c, 1), dtype=dt, device="cuda:0")
                nodes = [z(n), z(n), z(n), z(n), z(n, torch.int32), z(n, torch.int32), z(n), z(n), z(n, torch.uint8)]
                links = [z(2 * n + 1), z(m), z(m), z(m), z(m)]
                un = [z(u + 1), z(n), z(nc, torch.uint8), z(u), z(u, torch.uint8)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h.nodes_raw(*[t.data_ptr() for t in nodes], capacity=n)
                h.links_raw(*[t.data_ptr() for t in links], capacity=m)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                h.unitigs_raw(fm, 1, *[t.data_ptr() for t in un], capacity_unitigs=u, capacity_nodes=n, capacity_cells=nc)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                return nodes + links + un, t1 - t0, t2 - t1

            ref, times = None, {label: [] for label, _ in forms}
            for label, form in forms:                        # warm-up, and both forms give the same tables
                h, _ = create(form)
                got, _, _ = tables(h, form)
                h.close()
                if ref is None:
                    ref = got
                assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
            del got, ref
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
                    say("k = %d: %d nodes (%d rigid, %d palindromes) of %d distinct k-mers, %d edges, %d half-edges, %d hairpins, max end degree %d, %d unitigs "
                        "(%d circular, longest %d nodes), %d cells; %d jumping rounds; steps: mate pass %d backward %d forward, edge search %d backward; "
                        "handle %d bytes, scratch %d bytes"
                        % (k, i["n_nodes"], i["n_rigid"], i["n_palindromes"], i["n_distinct"], i["n_edges"], i["n_half_edges"], i["n_hairpins"],
                           i["max_end_degree"], i["n_unitigs"], i["n_circular"], i["longest_unitig"], i["n_cells"], i["jump_rounds"],
                           i["mate_backward_steps"], i["forward_steps"], i["edge_backward_steps"], i["handle_bytes"], i["scratch_bytes"]))
                ctx.profile_enable(True)
                _, t_copy, t_cells = tables(h, form)
                gw = grouped(ctx.profile())
                ctx.profile_enable(False)
                steps = h.info()["cells_forward_steps"]
                h.close()
                ts = sorted(times[label])
                say("  %-7s: create median %9.2f ms  min %9.2f  max %9.2f | kernels: node passes %8.2f, mate pass %8.2f, edge search %8.2f, merge %7.2f "
                    "(its kernels %7.3f), unitigs %7.2f, rest %6.2f ms | nodes + links %7.2f ms, unitigs with cells %7.2f ms (first cells and walks %7.3f, "
                    "tail cells %6.3f ms, %d forward steps)"
                    % (label, statistics.median(ts) * 1e3, ts[0] * 1e3, ts[-1] * 1e3, gr["node passes"], gr["mate pass"], gr["edge search"],
                       gr["merge kernels"] + gr["merge rest"], gr["merge kernels"], gr["unitigs"], gr["rest"], t_copy * 1e3, t_cells * 1e3,
                       gw["first cells"], gw["tail cells"], steps))
            set_form(None)
            if args.route_b:
                assert route_b(torch, np, fm, k, say) == i["n_half_edges"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--lib", default=None, help="a development library (tools/build_dev.sh): the generic forms are measured too")
    ap.add_argument("--route-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_cdebruijn", "cdebruijn.txt"))
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
        say("grlbwt_cdebruijn_*: create and the writers, the new kernels (default) against their generic forms (GRLBWT_DEV_CDEBRUIJN=f) on %s%s"
            % (torch.cuda.get_device_name(0), "; collections cut to a sixteenth (--small)" if args.small else ""))
    measure(args.leg, args, say)


if __name__ == "__main__":
    main()
