"""Shared by tests/test_fm_debruijn_sim.py (serial stand-in) and tests/test_fm_debruijn_gpu.py (HIP library): the compacted de Bruijn
graph of a collection from its FM index (grlbwt_debruijn_*).

Expected values share no code with the engine: a Python Counter of the k- and (k + 1)-windows of the rank-coded strings, sorted
tuples for the node ids, a dictionary walk for the unitigs, cycles started at their smallest id.  Cross-checks against the index:
the node table is FmIndex.kmers with the same filter, and FmIndex.count of an edge's k + 1 cells is (row, row + weight).

The inputs are sized from the tiles the library reports (info() of a first tiny call, and the row tile of the passes), never from
constants.  Every output buffer has guard bytes right behind the entries the call may write."""
import ctypes as C
from collections import Counter

import numpy as np

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import kmer_cases as kc
from tests import lcp_cases as lc
from tests import merge_cases as mc

EINVAL = -22
DT = fc.DT
FILL = fc.FILL
SMALL = ["twice", "one_string", "one_empty_string", "empty_strings", "rare_symbol", "two_bytes", "sigma_256", "wide_u64"]
NODE_TARGETS = ["tile_minus_1", "tile", "tile_plus_1", "three_tiles_17"]
CELL_TARGETS = NODE_TARGETS


# ------------------------------------------------------------------ expected values
class Coll:
    """a collection as rank-coded strings (tuples; the separator's rank 0 is in none of them) and the ranks' values"""

    def __init__(self, cells, w):
        self.cells, self.w = np.asarray(cells, dtype=DT[w]), w
        self.n = len(self.cells)
        vals, inv = np.unique(self.cells, return_inverse=True)
        assert int(vals[0]) == int(self.cells[-1])
        self.vals = vals.astype(np.uint64)
        self.strings = [tuple(int(v) for v in s) for s in lc.split(inv.astype(np.int64))]
        self.n_strings = len(self.strings)
        self.longest = max(len(s) for s in self.strings)
        self._win = {}

    def windows(self, k):
        if k not in self._win:
            cnt = Counter()
            if k <= self.longest:
                for s in self.strings:
                    cnt.update(s[j:j + k] for j in range(len(s) - k + 1))
            self._win[k] = cnt
        return self._win[k]


class Graph:
    """the graph by definition"""

    def __init__(self, col, k, min_count=1, max_count=0):
        ck, ck1 = col.windows(k), col.windows(k + 1)
        self.n_distinct = len(ck)
        keep = lambda c: c >= max(min_count, 1) and (not max_count or c <= max_count)
        self.keys = sorted(x for x, c in ck.items() if keep(c))
        n = self.n = len(self.keys)
        ident = {x: i for i, x in enumerate(self.keys)}
        self.count = np.array([ck[x] for x in self.keys], dtype=np.uint64)
        edges = sorted((ident[x[1:]], ident[x[:-1]], c, x) for x, c in ck1.items() if x[1:] in ident and x[:-1] in ident)
        self.to = [e[0] for e in edges]
        self.frm = np.array([e[1] for e in edges], dtype=np.uint64)
        self.weight = np.array([e[2] for e in edges], dtype=np.uint64)
        self.edge_keys = [e[3] for e in edges]
        self.indeg = np.bincount(self.to, minlength=n).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
        self.outdeg = np.bincount(self.frm.astype(np.int64), minlength=n).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
        self.in_offsets = np.concatenate([[0], np.cumsum(self.indeg, dtype=np.uint64)]).astype(np.uint64)
        # for a fixed `to`, ascending `from` is ascending first cell of `from`
        assert all(a[0] < b[0] or self.keys[a[1]][0] < self.keys[b[1]][0] for a, b in zip(edges, edges[1:]))
        succ, link = {}, {}
        for t, f, _, _ in edges:
            if self.outdeg[f] == 1 and self.indeg[t] == 1:
                succ[f], link[t] = t, f
        seen, paths = set(), []
        for h in [v for v in range(n) if v not in link] + list(range(n)):      # the heads first; what is left lies on cycles
            if h in seen:
                continue
            path, v = [h], h
            seen.add(h)
            while v in succ and succ[v] not in seen:
                v = succ[v]
                path.append(v)
                seen.add(v)
            circular = h in link
            assert not circular or (succ[v] == h and h == min(path))
            paths.append((path, circular))
        paths.sort(key=lambda p: p[0][0])
        assert sorted(v for p, _ in paths for v in p) == list(range(n))             # every node lies in exactly one unitig
        self.unitigs = [p for p, _ in paths]
        self.circular = np.array([c for _, c in paths], dtype=np.uint8)
        self.node_offsets = np.concatenate([[0], np.cumsum([len(p) for p in self.unitigs], dtype=np.uint64)]).astype(np.uint64)
        self.unitig_weight = np.array([int(sum(int(self.count[v]) for v in p)) for p in self.unitigs], dtype=np.uint64)
        self.unitig_of = np.zeros(n, dtype=np.uint64)
        self.rank_of = np.zeros(n, dtype=np.uint64)
        cells = []
        for j, p in enumerate(self.unitigs):
            for r, v in enumerate(p):
                self.unitig_of[v], self.rank_of[v] = j, r
            c = list(self.keys[p[0]]) + [self.keys[v][-1] for v in p[1:]]
            assert len(c) == k + len(p) - 1 and all(tuple(c[r:r + k]) == self.keys[v] for r, v in enumerate(p))
            cells += c
        self.cells = col.vals[np.array(cells, dtype=np.int64)] if cells else np.zeros(0, dtype=np.uint64)
        self.k, self.col = k, col
        assert len(self.cells) == n + len(self.unitigs) * (k - 1)


# ------------------------------------------------------------------ the tiles and the inputs sized by them
_tiles = {}


def tiles(ctx, mem, lib, flags):
    """(row tile of the passes, tile_nodes, tile_cells) from a first tiny call"""
    key = (lib, flags)
    if key not in _tiles:
        T = kc.tiles(ctx, mem, lib, flags)[0]
        blob = mc.build(lib, flags, np.frombuffer(b"AC\nA\n", dtype=np.uint8), 1)
        keep, p = mem.put(blob)
        with engine.FmIndex(ctx, p, len(blob)) as fm, fm.de_bruijn(1) as g:
            i = g.info()
        assert (i["n_nodes"], i["n_edges"], i["n_unitigs"]) == (2, 1, 1), i
        assert i["tile_nodes"] >= 64 and i["tile_cells"] >= 64, i
        _tiles[key] = (T, i["tile_nodes"], i["tile_cells"])
    return _tiles[key]


def target(name, t):
    return {"tile_minus_1": t - 1, "tile": t, "tile_plus_1": t + 1, "three_tiles_17": 3 * t + 17}[name]


def prefix_with_nodes(cells, k, min_count, want):
    """the shortest prefix of the collection's cells (closed with the separator) that has `want` k-mers of count >= min_count:
    a further cell adds at most one window, so every number up to the whole collection's is met"""
    sep, cnt, nodes, run = int(cells[-1]), Counter(), 0, []
    for i, c in enumerate(cells):
        if int(c) == sep:
            run = []
            continue
        run = (run + [int(c)])[-k:]
        if len(run) == k:
            x = tuple(run)
            cnt[x] += 1
            nodes += cnt[x] == min_count
            if nodes == want:
                return np.concatenate([cells[:i + 1], cells[-1:]])
    raise AssertionError("the collection has only %d such %d-mers, not %d" % (nodes, k, want))


_colls = {}


def coll_of(key, make):
    if key not in _colls:
        cells, w = make()
        _colls[key] = Coll(cells, w)
    return _colls[key]


def open_coll(ctx, flags, mem, lib, col, **kw):
    blob = mc.build(lib, flags, col.cells, col.w)
    keep, img = mem.put(blob)
    return engine.FmIndex(ctx, img, len(blob), **kw)


def text(strs, w=1):
    return mc.text([np.frombuffer(s.encode(), dtype=np.uint8) for s in strs], 10, 1).astype(DT[w]), w


# ------------------------------------------------------------------ one graph, guarded outputs, everything checked
def read_all(g, fm, mem, w, cells=True):
    """all three writers with buffers of exactly the reported size, guards right behind"""
    i = g.info()
    n, m, u, nc = i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_cells"]
    out = {}
    nb = [("lo", 8), ("count", 8), ("in_degree", 4), ("out_degree", 4), ("unitig", 8), ("rank", 8)]
    bufs = [mem.out(n * b) for _, b in nb]
    g.nodes_raw(*[p for _, p in bufs], capacity=n)
    for (name, b), (buf, _) in zip(nb, bufs):
        out[name] = mem.body(buf, n * b).view(np.uint64 if b == 8 else np.uint32)
    eb = [("in_offsets", n + 1), ("from", m), ("weight", m), ("row", m)]
    bufs = [mem.out(8 * c) for _, c in eb]
    g.edges_raw(*[p for _, p in bufs], capacity=m)
    for (name, c), (buf, _) in zip(eb, bufs):
        out[name] = mem.body(buf, 8 * c).view(np.uint64)
    ub = [("node_offsets", 8 * (u + 1)), ("nodes", 8 * n), ("cells", nc * w if cells else 0), ("unitig_weight", 8 * u), ("circular", u)]
    bufs = [mem.out(c) for _, c in ub]
    ptr = [p for _, p in bufs]
    g.unitigs_raw(fm if cells else None, w, ptr[0], ptr[1], ptr[2] if cells else None, ptr[3], ptr[4], u, n, nc)
    for (name, c), (buf, _) in zip(ub, bufs):
        out[name] = mem.body(buf, c).view(DT[w] if name == "cells" else np.uint8 if name == "circular" else np.uint64)
    return i, out


def invariants(i, o):
    """what holds on any image: CSR offsets, the degrees' sums, every node in one unitig at a place of its own"""
    n, m, u = i["n_nodes"], i["n_edges"], i["n_unitigs"]
    off = o["in_offsets"]
    assert int(off[0]) == 0 and int(off[-1]) == m and bool(np.all(off[1:] >= off[:-1]))
    assert np.array_equal(np.diff(off.astype(np.int64)), o["in_degree"].astype(np.int64))
    assert int(o["in_degree"].sum()) == m == int(o["out_degree"].sum())
    assert np.array_equal(np.bincount(o["from"].astype(np.int64), minlength=n)[:n], o["out_degree"].astype(np.int64)) if n else m == 0
    uo = o["node_offsets"]
    assert int(uo[0]) == 0 and int(uo[-1]) == n and bool(np.all(uo[1:] > uo[:-1]))
    assert sorted(int(v) for v in o["nodes"]) == list(range(n))
    slot = uo[o["unitig"].astype(np.int64)] + o["rank"] if n else np.zeros(0, dtype=np.uint64)
    assert np.array_equal(o["nodes"][slot.astype(np.int64)], np.arange(n, dtype=np.uint64))
    assert i["n_cells"] == (n + u * (i["k"] - 1) if n else 0)
    assert i["n_circular"] == int(o["circular"].sum()) and i["longest_unitig"] == (int(np.diff(uo.astype(np.int64)).max()) if u else 0)
    assert i["max_in_degree"] == (int(o["in_degree"].max()) if n else 0) and i["max_out_degree"] == (int(o["out_degree"].max()) if n else 0)
    first = o["nodes"][uo[:-1].astype(np.int64)] if u else np.zeros(0, dtype=np.uint64)
    assert bool(np.all(first[1:] > first[:-1]))                                 # unitigs in ascending first node


def check(fm, mem, col, k, min_count=1, max_count=0, w=None):
    """the graph of (k, min_count, max_count) against the definition; returns (info, outputs, expected)"""
    w = w or col.w
    e = Graph(col, k, min_count, max_count)
    with fm.de_bruijn(k, min_count, max_count) as g:
        i, o = read_all(g, fm, mem, w)
    n, m, u = e.n, len(e.frm), len(e.unitigs)
    assert (i["k"], i["n_rows"], i["n_strings"], i["n_distinct"]) == (k, col.n, col.n_strings, e.n_distinct), i
    assert (i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_circular"]) == (n, m, u, int(e.circular.sum())), (i, n, m, u)
    assert i["n_cells"] == len(e.cells) and i["longest_unitig"] == max([len(p) for p in e.unitigs] + [0]), i
    assert i["passes"] <= max(k - 1, 0) and i["passes"] + i["length_passes"] <= min(k - 1, col.longest + 1), i
    assert i["backward_steps"] >= 2 * n and i["backward_steps"] % 2 == 0, i
    assert i["jump_rounds"] <= 2 * (max(n - 1, 0).bit_length() + 1), i
    assert i["handle_bytes"] >= 4 * (5 * n + 3 * m) and (i["scratch_bytes"] >= col.n // 2 or col.n == 0), i
    invariants(i, o)
    lo, count, cells = fm.kmers(k, min_count, max_count, cell_bytes=8) if n else (np.zeros(0, dtype=np.uint64),) * 3     # the node table
    assert np.array_equal(o["lo"], lo) and np.array_equal(o["count"], count) and np.array_equal(count, e.count)
    if n:
        assert np.array_equal(cells, col.vals[np.array(e.keys, dtype=np.int64).reshape(n, k)])
    for name, want in (("in_degree", e.indeg), ("out_degree", e.outdeg), ("in_offsets", e.in_offsets), ("from", e.frm), ("weight", e.weight),
                       ("unitig", e.unitig_of), ("rank", e.rank_of), ("node_offsets", e.node_offsets), ("unitig_weight", e.unitig_weight),
                       ("circular", e.circular), ("cells", e.cells.astype(DT[w]))):
        assert np.array_equal(o[name], want), (name, k, min_count, max_count, np.flatnonzero(o[name] != want)[:5])
    assert [int(v) for v in o["nodes"]] == [v for p in e.unitigs for v in p]
    if m:                                                                      # what grlbwt_fm_count answers for the edges' cells
        pats = [[int(col.vals[c]) for c in x] for x in e.edge_keys]
        assert fc.count(fm, mem, pats, col.w) == [(int(r), int(r + wt)) for r, wt in zip(o["row"], o["weight"])]
    return i, o, e


# ------------------------------------------------------------------ the cases
def rows_coll(ctx, flags, mem, lib):
    T = tiles(ctx, mem, lib, flags)[0]
    return lc.cases(T)["rows_three_tiles_17"]


def run_nodes_around_the_edge_tile(ctx, flags, mem, lib, name):
    """tile_nodes - 1, tile_nodes, tile_nodes + 1 and 3 tile_nodes + 17 nodes out of rows_three_tiles_17, at k = 5 and k = 6: the
    collection is cut to the prefix that has that many k-mers under the filter, and max_count takes the most frequent ones away"""
    T, TN, _ = tiles(ctx, mem, lib, flags)
    base = rows_coll(ctx, flags, mem, lib).cells
    want = target(name, TN)
    done = 0
    for k, min_count in ((5, 1), (5, 2), (6, 1), (6, 2)):
        full = Coll(base, 1).windows(k)
        if sum(1 for c in full.values() if c >= min_count) < want:
            continue                                                            # (4^5 k-mers at k = 5: the larger targets are k = 6's)
        col = coll_of(("nodes", T, TN, name, k, min_count), lambda: (prefix_with_nodes(base, k, min_count, want), 1))
        with open_coll(ctx, flags, mem, lib, col) as fm:
            i, _, e = check(fm, mem, col, k, min_count)
            assert i["n_nodes"] == want
            top = int(e.count.max())
            i, _, _ = check(fm, mem, col, k, min_count, top - 1)
            assert 0 < i["n_nodes"] < want
        done += 1
    assert done >= {"three_tiles_17": 1, "tile_plus_1": 2}.get(name, 3), (name, done)      # (k = 5 has 4^5 k-mers at the most)


def cells_coll(TC, name):
    def make():
        rng = np.random.default_rng(20261021 + target(name, TC))
        return mc.text([mc.ACGT[rng.integers(0, 4, size=target(name, TC))]], 10, 1), 1
    return coll_of(("cells", TC, name), make)


def run_cells_around_the_decode_tile(ctx, flags, mem, lib, name, k=20):
    """one random string of tile_cells - 1 .. 3 tile_cells + 17 cells whose k-mers are all different: one unitig of that many
    cells, ranked over several jumping rounds"""
    TC = tiles(ctx, mem, lib, flags)[2]
    col = cells_coll(TC, name)
    assert max(col.windows(k).values()) == 1
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, _ = check(fm, mem, col, k)
        assert (i["n_unitigs"], i["n_cells"], i["n_circular"]) == (1, target(name, TC), 0), i
        assert i["jump_rounds"] >= 2, i
        assert np.array_equal(o["cells"], col.cells[:-1])


def run_cycles(ctx, flags, mem, lib):
    T, TN, _ = tiles(ctx, mem, lib, flags)

    def long_cycle():
        block = mc.ACGT[np.random.default_rng(20261022).integers(0, 4, size=TN + 5)]
        return mc.text([np.concatenate([block, block, block])], 10, 1), 1
    col = coll_of(("cycle", TN), long_cycle)
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, e = check(fm, mem, col, 12)
        assert (i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_circular"], i["longest_unitig"]) == (TN + 5, TN + 5, 1, 1, TN + 5), i
        assert bool(np.all(o["in_degree"] == 1)) and bool(np.all(o["out_degree"] == 1)) and int(o["nodes"][0]) == 0
        assert i["jump_rounds"] > (TN + 4).bit_length()                        # the cycle rounds ran
    col = coll_of("acg3", lambda: text(["ACGACGACG"]))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, _ = check(fm, mem, col, 3)
        assert (i["n_nodes"], i["n_unitigs"], i["n_circular"]) == (3, 1, 1) and [int(v) for v in o["nodes"]] == [0, 1, 2], i
    col = coll_of(("loop", T), lambda: (np.concatenate([np.repeat(mc.ACGT[:1], 3 * T), [10]]).astype(np.uint8), 1))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        for k in (1, 7, 70):
            i, o, _ = check(fm, mem, col, k)
            assert (i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_circular"]) == (1, 1, 1, 1), i
            assert int(o["weight"][0]) == 3 * T - k and int(o["from"][0]) == 0


def run_branches(ctx, flags, mem, lib):
    for key, strs, ks in (("fork", ["ACGTACCA", "ACGTAGGT"], (2, 3, 4)), ("join", ["CCATTGCA", "GGTTTGCA"], (2, 3, 4)),
                          ("bubble", ["ACGTTCATGGA", "ACGTTGATGGA"], (2, 3, 4, 5)), ("against", ["TTACGGA", "TTACCGA"], (2,))):
        col = coll_of(key, lambda: text(strs))
        with open_coll(ctx, flags, mem, lib, col) as fm:
            for k in ks:
                i, o, e = check(fm, mem, col, k)
                assert i["max_in_degree"] >= 1 and i["n_unitigs"] > 1
            if key == "against":
                assert [6, 5, 0] in e.unitigs                                   # a unitig that runs against the id order

    def reads():
        rng = np.random.default_rng(20261023)
        genome = mc.ACGT[rng.integers(0, 4, size=2000)]
        out = []
        for s in rng.integers(0, 2000 - 30 + 1, size=2000 * 8 // 30):
            r = genome[s:s + 30].copy()
            out.append(r)
        flat = np.concatenate(out)
        for x in range(25, len(flat), 50):                                      # one substituted cell per 50
            flat[x] = mc.ACGT[(int(np.flatnonzero(mc.ACGT == flat[x])[0]) + 1 + x % 3) % 4]
        return mc.text([flat[j:j + 30] for j in range(0, len(flat), 30)], 10, 1), 1
    col = coll_of("reads", reads)
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i1, _, _ = check(fm, mem, col, 9)
        i2, _, _ = check(fm, mem, col, 9, 2)
        assert i2["n_nodes"] < i1["n_nodes"] and i2["n_unitigs"] < i1["n_unitigs"] and i2["longest_unitig"] > i1["longest_unitig"], (i1, i2)


def run_filters(ctx, flags, mem, lib):
    col = coll_of("split", lambda: text(["ACCGTATTGC", "GGCGTATCAA"]))          # GTAT occurs twice, in the middle of both paths
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i1, _, e1 = check(fm, mem, col, 4)
        i2, _, e2 = check(fm, mem, col, 4, 1, 1)
        assert i2["n_nodes"] < i1["n_nodes"] and i2["n_unitigs"] == 4 and i2["max_in_degree"] == i2["max_out_degree"] == 1, (i1, i2)
        for mn, mx in ((3, 0), (5, 9)):                                        # every node filtered out: an empty graph
            i, o, _ = check(fm, mem, col, 4, mn, mx)
            assert (i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_cells"]) == (0, 0, 0, 0) and i["n_distinct"] > 0


def run_values_of_k(ctx, flags, mem, lib):
    col = coll_of("values_of_k", lambda: text(["ACGTACGGT", "ACGT", "", "TTGACGTAC"]))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        check(fm, mem, col, 1)
        i, _, _ = check(fm, mem, col, col.longest)
        assert i["n_nodes"] >= 1 and i["n_edges"] == 0
        for k in (col.longest + 1, 10 ** 6, 2 ** 63):
            i, _, _ = check(fm, mem, col, k)
            assert (i["n_nodes"], i["n_cells"], i["n_distinct"]) == (0, 0, 0)


def run_small(ctx, flags, mem, lib, name):
    T = tiles(ctx, mem, lib, flags)[0]
    c = lc.cases(T)[name]
    col = coll_of(("small", T, name), lambda: (c.cells, c.w))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        for k in (1, 2, 3, max(col.longest, 1)):
            i, _, _ = check(fm, mem, col, k)
            check(fm, mem, col, k, 2)
        if name == "sigma_256":
            j = check(fm, mem, col, 1)[0]                                       # every node tries many candidate symbols
            assert j["n_strings"] > 5 and j["backward_steps"] > 2 * 16 * j["n_nodes"], j
        if name in ("one_empty_string", "empty_strings"):
            assert check(fm, mem, col, 1)[0]["n_nodes"] == 0
        if name == "two_bytes":
            check(fm, mem, col, 2, w=4)
        if name == "wide_u64":                                                 # values as values; a narrower width is refused, nothing written
            assert int(col.vals.max()) == 2 ** 63 + 11
            with fm.de_bruijn(2) as g:
                i = g.info()
                for w in (1, 2, 4):
                    bufs = [mem.out(8 * (i["n_unitigs"] + 1)), mem.out(i["n_cells"] * w)]
                    msg = fc.einval(lambda: g.unitigs_raw(fm, w, bufs[0][1], None, bufs[1][1], None, None, i["n_unitigs"], 0, i["n_cells"]))
                    assert "does not fit" in msg and all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs)
                    g.unitigs_raw(None, w, bufs[0][1], capacity_unitigs=i["n_unitigs"])      # without the cells the width is not looked at
                    mem.body(bufs[0][0], 8 * (i["n_unitigs"] + 1))
                assert len(g.nodes()["lo"]) == i["n_nodes"] and len(g.edges()[1]) == i["n_edges"]


def run_outputs_and_sizing(ctx, flags, mem, lib):
    """every array of every writer alone; each capacity one short is EINVAL with all guards intact; the array-returning forms"""
    col = coll_of("reads_small", lambda: text(["ACGTACGGTTACGTAGGT", "TTACGGATTACCGA", "ACGTACG", "GGTTACGTAG"]))
    L = ctx.L
    with open_coll(ctx, flags, mem, lib, col) as fm:
        _, o, e = check(fm, mem, col, 3)
        with fm.de_bruijn(3) as g:
            i = g.info()
            n, m, u, nc = i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_cells"]
            assert n > 3 and m > 3 and u > 1
            calls = [
                (lambda p, c: g.nodes_raw(*p, capacity=c[0]), [("lo", 8 * n), ("count", 8 * n), ("in_degree", 4 * n), ("out_degree", 4 * n),
                                                               ("unitig", 8 * n), ("rank", 8 * n)], [n], lambda j: 0),
                (lambda p, c: g.edges_raw(*p, capacity=c[0]), [("in_offsets", 8 * (n + 1)), ("from", 8 * m), ("weight", 8 * m), ("row", 8 * m)],
                 [m], lambda j: 0),
                (lambda p, c: g.unitigs_raw(fm, 1, *p, capacity_unitigs=c[0], capacity_nodes=c[1], capacity_cells=c[2]),
                 [("node_offsets", 8 * (u + 1)), ("nodes", 8 * n), ("cells", nc), ("unitig_weight", 8 * u), ("circular", u)], [u, n, nc],
                 lambda j: (0, 1, 2, 0, 0)[j]),
            ]
            for fn, arrays, caps, cap_of in calls:
                fc.einval(lambda: fn([None] * len(arrays), caps))                # no array at all
                for j, (name, nbytes) in enumerate(arrays):
                    buf, ptr = mem.out(nbytes)
                    args = [ptr if x == j else None for x in range(len(arrays))]
                    fn(args, caps)                                               # the array alone
                    dt = np.uint32 if "degree" in name else np.uint8 if name in ("cells", "circular") else np.uint64
                    assert np.array_equal(mem.body(buf, nbytes).view(dt), o[name].astype(dt)), name
                    buf, ptr = mem.out(nbytes)                                   # its capacity one short
                    args = [ptr if x == j else None for x in range(len(arrays))]
                    short = [c - 1 if x == cap_of(j) else c for x, c in enumerate(caps)]
                    msg = fc.einval(lambda: fn(args, short))
                    assert "GRLBWT" not in msg and bool(np.all(mem.get(buf) == FILL)), name
            rc = L.grlbwt_debruijn_nodes(ctx._h, None, None, None, None, None, None, None, 0)
            assert rc == EINVAL
            nodes, edges, un = g.nodes(), g.edges(), g.unitigs()
            for name in ("lo", "count", "in_degree", "out_degree", "unitig", "rank"):
                assert np.array_equal(nodes[name], o[name]) and nodes[name].dtype == o[name].dtype, name
            assert all(np.array_equal(a, o[b]) for a, b in zip(edges, ("in_offsets", "from", "weight", "row")))
            assert np.array_equal(un["node_offsets"], o["node_offsets"]) and np.array_equal(un["nodes"], o["nodes"])
            assert np.array_equal(un["weight"], o["unitig_weight"]) and np.array_equal(un["circular"], o["circular"])
            assert un["cells"].dtype == np.uint8 and np.array_equal(un["cells"], o["cells"])
            assert np.array_equal(un["cell_offsets"], o["node_offsets"] + np.arange(u + 1, dtype=np.uint64) * np.uint64(2))
            for j, p in enumerate(e.unitigs):                                   # the closed form finds every unitig's cells
                a = int(un["cell_offsets"][j])
                assert len(un["cells"][a:int(un["cell_offsets"][j + 1])]) == 3 + len(p) - 1
            assert "cells" not in g.unitigs(cells=False)


def run_refusals(ctx, flags, mem, lib):
    col = coll_of("reads_small", lambda: text(["ACGTACGGTTACGTAGGT", "TTACGGATTACCGA", "ACGTACG", "GGTTACGTAG"]))
    # the same strings in another order: as many rows, runs, strings and symbols, so only the fingerprint tells the indexes apart
    other = coll_of("other", lambda: text(["GGTTACGTAG", "ACGTACGGTTACGTAGGT", "ACGTACG", "TTACGGATTACCGA"]))
    L = ctx.L
    with open_coll(ctx, flags, mem, lib, col) as fm:
        fc.einval(lambda: fm.de_bruijn(0))                                      # k = 0
        fc.einval(lambda: fm.de_bruijn(3, 5, 4))                                # min_count > max_count != 0
        fc.einval(lambda: engine.DeBruijn(fm, 3, flags=1))                      # flags other than 0
        fm.de_bruijn(3, 5, 0).close()
        h = C.c_void_p(7)
        assert L.grlbwt_debruijn_create(ctx._h, None, 3, 1, 0, 0, C.byref(h)) == EINVAL and not h.value        # a null index
        assert L.grlbwt_debruijn_create(ctx._h, fm._h, 3, 1, 0, 0, None) == EINVAL
        assert L.grlbwt_debruijn_info_get(None, None) == EINVAL
        assert L.grlbwt_debruijn_destroy(ctx._h, None) == 0
        with fm.de_bruijn(3) as g, open_coll(ctx, flags, mem, lib, other) as fm2:
            i = g.info()
            a, b = fm.info(), fm2.info()
            assert all(a[x] == b[x] for x in ("n_syms", "n_runs", "n_strings", "sigma", "separator")), (a, b)
            buf, ptr = mem.out(i["n_cells"])
            msg = fc.einval(lambda: g.unitigs_raw(fm2, 1, cells_ptr=ptr, capacity_cells=i["n_cells"]))          # a second index
            assert "not the index" in msg and "GRLBWT" not in msg and bool(np.all(mem.get(buf) == FILL))
            fc.einval(lambda: g.unitigs_raw(None, 1, cells_ptr=ptr, capacity_cells=i["n_cells"]))               # the cells without an index
            for w in (0, 3, 16):
                fc.einval(lambda: g.unitigs_raw(fm, w, cells_ptr=ptr, capacity_cells=i["n_cells"]))
            assert bool(np.all(mem.get(buf) == FILL))
            g.unitigs_raw(fm, 1, cells_ptr=ptr, capacity_cells=i["n_cells"])
            mem.body(buf, i["n_cells"])
    bad = ic.make_image(1, 1, [10, 65], [1, 2])              # not the BWT of a collection: the row of the second A is LF of itself
    keep, img = mem.put(bad)
    with engine.FmIndex(ctx, img, len(bad)) as fm:
        msg = fc.einval(lambda: fm.de_bruijn(3))
        assert "not the BWT of a collection" in msg, msg


def run_index_unchanged(ctx, flags, mem, lib):
    col = fc.COLS["dna"]
    pats = fc.collection_patterns(col)
    blob = fc.image_of(lib, col, flags)
    c = coll_of("fc_dna", lambda: (col.data, 1))
    for kw in ({}, {"locate": True}, {"locate": True, "checkpoints": True, "sample_bits": 3}, {"locate": True, "extract": True}):
        keep, img = mem.put(blob)
        fm = engine.FmIndex(ctx, img, len(blob), **kw)
        del keep
        before, counts = fm.info(), fc.count(fm, mem, pats, 1)
        buf, ptr = mem.out(c.n)
        lcp_before = (fm.lcp(0, 1, ptr), mem.body(buf, c.n).tobytes())
        check(fm, mem, c, 3)
        _, o, _ = check(fm, mem, c, 7, 2)
        assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts, kw
        buf, ptr = mem.out(c.n)
        after = (fm.lcp(0, 1, ptr), mem.body(buf, c.n).tobytes())
        assert lcp_before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(lcp_before[0], after[0]))
        g = fm.de_bruijn(7, 2)
        fm.close()                                                              # the handle survives its index
        nodes, edges = g.nodes(), g.edges()
        assert np.array_equal(nodes["lo"], o["lo"]) and np.array_equal(nodes["unitig"], o["unitig"])
        assert np.array_equal(edges[0], o["in_offsets"]) and np.array_equal(edges[1], o["from"]) and np.array_equal(edges[3], o["row"])
        assert len(g.unitigs(cells=False)["nodes"]) == len(o["nodes"])
        g.close()


def run_foreign(ctx, mem, c):
    """an image the engine did not make is refused or answered, and never runs past the guards; returns (answered, refused)"""
    blob = c.image()
    keep, img = mem.put(blob)
    try:
        fm = engine.FmIndex(ctx, img, len(blob))
    except engine.GrlbwtError as e:
        assert e.code == EINVAL, e
        return 0, 1
    done = refused = 0
    with fm:
        n = fm.info()["n_syms"]
        for k in (1, 2, 5):
            try:
                g = fm.de_bruijn(k)
            except engine.GrlbwtError as e:
                assert e.code == EINVAL, e
                refused += 1
                continue
            with g:
                i, o = read_all(g, fm, mem, 8)
                assert i["n_nodes"] <= n and i["n_edges"] <= n and i["n_nodes"] == fm.kmers_raw(k)
                invariants(i, o)
                assert bool(np.all(o["lo"][1:] > o["lo"][:-1])) and bool(np.all(o["lo"] + o["count"] <= n))
                assert bool(np.all(o["from"] < max(i["n_nodes"], 1))) and bool(np.all(o["row"] + o["weight"] <= n))
            done += 1
    return done, refused
