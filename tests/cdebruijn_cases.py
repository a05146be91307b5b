"""Shared by tests/test_fm_cdebruijn_sim.py (serial stand-in) and tests/test_fm_cdebruijn_gpu.py (HIP library): the strand-merged
compacted de Bruijn graph of a collection from its FM index (grlbwt_cdebruijn_*).

Expected values share no code with the engine: Python Counters of the k- and (k + 1)-windows of the strings as tuples of symbol
values, the reverse complement through a dict built from the pairs, the classes by a walk over the sorted k-mers, ends and
half-edges by the definitions of the header, unitigs by a dictionary walk with the normal form.  The model asserts that the
hairpins are exactly the windows that are their own reverse complement, and that every node lies in one unitig.  Cross-checks
against existing calls: the node table is FmIndex.canonical_kmers with the same arguments, FmIndex.count of every half-edge's
window read from its source end is (fwd_row, fwd_row + fwd_count), and FmIndex.de_bruijn on both-strand and on all-rigid inputs.

The inputs are sized from the tiles the library reports (info() of a first tiny call), never from constants.  Every output buffer
has guard bytes right behind the entries the call may write."""
import ctypes as C
from collections import Counter

import numpy as np

from grlbwt_amd import engine
from tests import debruijn_cases as dc
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import lcp_cases as lc
from tests import merge_cases as mc

EINVAL = -22
DT = fc.DT
FILL = fc.FILL
NONE = fc.NONE
DNA = ((65, 84), (67, 71))
TARGETS = ["tile_minus_1", "tile", "tile_plus_1", "three_tiles_17"]
NODE_COLS = (("lo", 8), ("count", 8), ("mate_lo", 8), ("total", 8), ("degree0", 4), ("degree1", 4), ("unitig", 8), ("rank", 8), ("orient", 1))
LINK_COLS = ("end_offsets", "other", "weight", "fwd_row", "fwd_count")
NPDT = {8: np.uint64, 4: np.uint32, 1: np.uint8}
target = dc.target
coll_of = dc.coll_of
open_coll = dc.open_coll
text = dc.text


# ------------------------------------------------------------------ expected values
class CGraph:
    """the graph by definition, over tuples of symbol values"""

    def __init__(self, col, k, min_count=1, max_count=0, pairs=None):
        vals = [int(v) for v in col.vals]
        ck, ck1 = Counter(), Counter()
        for s in col.strings:
            t = tuple(vals[c] for c in s)
            ck.update(t[j:j + k] for j in range(len(t) - k + 1))
            ck1.update(t[j:j + k + 1] for j in range(len(t) - k))
        comp = {}
        for a, b in (DNA if pairs is None else pairs):
            comp[int(a)], comp[int(b)] = int(b), int(a)
        self.comp = comp

        def rc(x):
            return None if any(v not in comp for v in x) else tuple(comp[v] for v in reversed(x))
        self.rc = rc
        self.n_distinct = len(ck)
        keep = lambda c: c >= max(min_count, 1) and (not max_count or c <= max_count)
        seen, self.keys, self.count, self.total, self.mate, ident = set(), [], [], [], [], {}
        for x in sorted(ck):                                        # ascending lo: the first member met is the representative
            if x in seen:
                continue
            r = rc(x)
            m = r if r is not None and r in ck else None
            seen |= {x} | ({m} if m else set())
            tot = ck[x] + (ck[m] if m and m != x else 0)
            if not keep(tot):
                continue
            v = len(self.keys)
            ident[x] = (v, False)
            if m and m != x:
                ident[m] = (v, True)
            self.keys.append(x); self.count.append(ck[x]); self.total.append(tot); self.mate.append(m)
        n = self.n = len(self.keys)
        self.pal = [rc(x) == x for x in self.keys]
        self.rigid = [rc(x) is None or rc(x) == x for x in self.keys]
        H, self.n_windows = {}, 0                                   # (source end, other end) -> [weight, the window read that way or None]

        def add(a, b, c, w):
            e = H.setdefault((a, b), [0, None])
            e[0] += c
            if w is not None:
                assert e[1] is None
                e[1] = w
        for w, c in ck1.items():
            p, s = w[:-1], w[1:]
            if p not in ident or s not in ident:
                continue
            self.n_windows += c
            (u, um), (v, vm) = ident[p], ident[s]
            a = 2 * u + (0 if um or self.pal[u] else 1)
            b = 2 * v + (1 if vm else 0)
            assert (a == b) == (rc(w) == w), w                      # the hairpins are exactly the self-reverse-complementary windows
            add(a, b, c, w)
            if a != b:
                add(b, a, c, None)
        self.H = H
        self.links = sorted(H)
        self.n_hairpins = sum(1 for a, b in self.links if a == b)
        assert (len(self.links) + self.n_hairpins) % 2 == 0 and all((b, a) in H and H[(b, a)][0] == H[(a, b)][0] for a, b in self.links)
        self.n_edges = (len(self.links) + self.n_hairpins) // 2
        assert sum(H[e][0] for e in self.links if e[0] <= e[1]) == self.n_windows
        deg = np.zeros(2 * n + 1, dtype=np.int64)
        for a, _ in self.links:
            deg[a] += 1
        assert all(deg[2 * v + 1] == 0 for v in range(n) if self.pal[v])
        self.deg = deg[:2 * n]
        self.end_offsets = np.concatenate([[0], np.cumsum(self.deg)]).astype(np.uint64)
        only = {}
        for a, b in self.links:
            only[a] = b

        def partner(a):
            if deg[a] != 1:
                return None
            b = only[a]
            if b == a or deg[b] != 1 or self.rigid[a >> 1] or self.rigid[b >> 1]:
                return None
            return b
        succ = lambda x: partner(x ^ 1)                             # reading (v, o) leaves through end 1 - o and lands on (w, f)
        pred = lambda x: None if partner(x) is None else partner(x) ^ 1
        self.partner = partner
        done, paths = set(), []
        for v in range(n):                                          # ascending: v is the smallest node of its unitig
            if v in done:
                continue
            x, circular = 2 * v, False
            while pred(x) is not None:
                x = pred(x)
                if x == 2 * v:
                    circular = True
                    break
            path = [x]
            while succ(path[-1]) is not None and succ(path[-1]) != path[0]:
                path.append(succ(path[-1]))
            assert circular == (succ(path[-1]) == path[0])
            if not circular and len(path) > 1 and (path[-1] >> 1) < (path[0] >> 1):
                path = [y ^ 1 for y in reversed(path)]
            if not circular and len(path) == 1:
                path = [2 * v]
            assert path[0] >> 1 == v or not circular
            assert not (done & set(y >> 1 for y in path)) and len(set(y >> 1 for y in path)) == len(path)
            done |= set(y >> 1 for y in path)
            paths.append((path, circular))
        paths.sort(key=lambda p: p[0][0] >> 1)
        assert sorted(y >> 1 for p, _ in paths for y in p) == list(range(n))       # every node lies in exactly one unitig
        self.unitigs = [p for p, _ in paths]
        self.circular = np.array([c for _, c in paths], dtype=np.uint8)
        self.node_offsets = np.concatenate([[0], np.cumsum([len(p) for p in self.unitigs])]).astype(np.uint64)
        self.unitig_weight = np.array([sum(self.total[y >> 1] for y in p) for p in self.unitigs], dtype=np.uint64)
        self.unitig_of, self.rank_of, self.orient_of = (np.zeros(n, dtype=t) for t in (np.uint64, np.uint64, np.uint8))
        read = lambda y: self.keys[y >> 1] if not y & 1 else rc(self.keys[y >> 1])
        cells = []
        for j, p in enumerate(self.unitigs):
            for r, y in enumerate(p):
                self.unitig_of[y >> 1], self.rank_of[y >> 1], self.orient_of[y >> 1] = j, r, y & 1
            c = list(read(p[0])) + [read(y)[-1] for y in p[1:]]
            assert all(tuple(c[r:r + k]) == read(y) for r, y in enumerate(p))
            cells += c
        self.cells = np.array(cells, dtype=np.uint64)
        self.k, self.col = k, col
        assert len(self.cells) == n + len(self.unitigs) * (k - 1)

    def window(self, a, b):
        """the window of half-edge a -> b as read from a to b"""
        w = self.H[(a, b)][1]
        return w if w is not None else self.rc(self.H[(b, a)][1])


# ------------------------------------------------------------------ the tiles
_tiles = {}


def tiles(ctx, mem, lib, flags):
    """(tile_nodes, tile_cells) from a first tiny call"""
    key = (lib, flags)
    if key not in _tiles:
        blob = mc.build(lib, flags, np.frombuffer(b"AC\nA\n", dtype=np.uint8), 1)
        keep, p = mem.put(blob)
        with engine.FmIndex(ctx, p, len(blob)) as fm, fm.de_bruijn_canonical(1) as g:
            i = g.info()
        assert (i["n_nodes"], i["n_edges"], i["n_half_edges"], i["n_unitigs"], i["n_rigid"]) == (2, 1, 2, 1, 0), i
        assert i["tile_nodes"] >= 64 and i["tile_cells"] >= 64, i
        _tiles[key] = (i["tile_nodes"], i["tile_cells"])
    return _tiles[key]


def revcomp(s):
    return np.array([{65: 84, 84: 65, 67: 71, 71: 67}[int(v)] for v in s[::-1]], dtype=np.uint8)


# ------------------------------------------------------------------ one graph, guarded outputs, everything checked
def read_all(g, fm, mem, w, cells=True):
    """all three writers with buffers of exactly the reported size, guards right behind"""
    i = g.info()
    n, m, u, nc = i["n_nodes"], i["n_half_edges"], i["n_unitigs"], i["n_cells"]
    out = {}
    bufs = [mem.out(n * b) for _, b in NODE_COLS]
    g.nodes_raw(*[p for _, p in bufs], capacity=n)
    for (name, b), (buf, _) in zip(NODE_COLS, bufs):
        out[name] = mem.body(buf, n * b).view(NPDT[b])
    sizes = [2 * n + 1, m, m, m, m]
    bufs = [mem.out(8 * c) for c in sizes]
    g.links_raw(*[p for _, p in bufs], capacity=m)
    for name, c, (buf, _) in zip(LINK_COLS, sizes, bufs):
        out[name] = mem.body(buf, 8 * c).view(np.uint64)
    ub = [("node_offsets", 8 * (u + 1)), ("nodes", 8 * n), ("cells", nc * w if cells else 0), ("unitig_weight", 8 * u), ("circular", u)]
    bufs = [mem.out(c) for _, c in ub]
    ptr = [p for _, p in bufs]
    g.unitigs_raw(fm if cells else None, w, ptr[0], ptr[1], ptr[2] if cells else None, ptr[3], ptr[4], u, n, nc)
    for (name, c), (buf, _) in zip(ub, bufs):
        out[name] = mem.body(buf, c).view(DT[w] if name == "cells" else np.uint8 if name == "circular" else np.uint64)
    return i, out


def invariants(i, o):
    """what holds on any image: the CSR over the ends, the degrees, every node in one unitig at a place of its own"""
    n, m, u = i["n_nodes"], i["n_half_edges"], i["n_unitigs"]
    off = o["end_offsets"]
    assert len(off) == 2 * n + 1 and int(off[0]) == 0 and int(off[-1]) == m and bool(np.all(off[1:] >= off[:-1]))
    d = np.diff(off.astype(np.int64))
    assert np.array_equal(d[0::2], o["degree0"].astype(np.int64)) and np.array_equal(d[1::2], o["degree1"].astype(np.int64))
    assert i["max_end_degree"] == (int(d.max()) if n else 0)
    assert bool(np.all(o["other"] < max(2 * n, 1))) and m == 2 * i["n_edges"] - i["n_hairpins"]
    src = np.repeat(np.arange(2 * n, dtype=np.uint64), d) if n else np.zeros(0, dtype=np.uint64)
    assert int(np.count_nonzero(src == o["other"])) == i["n_hairpins"]
    for a in range(2 * n):                                                      # ascending other end inside a segment
        seg = o["other"][int(off[a]):int(off[a + 1])]
        assert bool(np.all(seg[1:] > seg[:-1]))
    back = set(zip(src.tolist(), o["other"].tolist()))
    assert all((b, a) in back for a, b in back)                                 # every half-edge has its reverse
    assert bool(np.all((o["fwd_row"] == NONE) == (o["fwd_count"] == 0))) and bool(np.all(o["fwd_count"] <= o["weight"]))
    uo = o["node_offsets"]
    assert int(uo[0]) == 0 and int(uo[-1]) == n and bool(np.all(uo[1:] > uo[:-1]))
    assert sorted(int(v) >> 1 for v in o["nodes"]) == list(range(n))
    slot = uo[o["unitig"].astype(np.int64)] + o["rank"] if n else np.zeros(0, dtype=np.uint64)
    assert np.array_equal(o["nodes"][slot.astype(np.int64)], 2 * np.arange(n, dtype=np.uint64) + o["orient"])
    assert i["n_cells"] == (n + u * (i["k"] - 1) if n else 0)
    assert i["n_circular"] == int(o["circular"].sum()) and i["longest_unitig"] == (int(np.diff(uo.astype(np.int64)).max()) if u else 0)
    first = o["nodes"][uo[:-1].astype(np.int64)] >> np.uint64(1) if u else np.zeros(0, dtype=np.uint64)
    assert bool(np.all(first[1:] > first[:-1]))                                 # unitigs in ascending first node
    assert int(o["unitig_weight"].sum()) == int(o["total"].sum())


def check(fm, mem, col, k, min_count=1, max_count=0, pairs=None, w=None):
    """the graph of (k, min_count, max_count, pairs) against the definition; returns (info, outputs, expected)"""
    w = w or col.w
    e = CGraph(col, k, min_count, max_count, pairs)
    with fm.de_bruijn_canonical(k, min_count, max_count, pairs) as g:
        i, o = read_all(g, fm, mem, w)
        assert i["cells_forward_steps"] == 0
        i = g.info()                                                            # (with the steps of the cells call)
    n, m, u = e.n, len(e.links), len(e.unitigs)
    assert (i["k"], i["n_rows"], i["n_strings"], i["n_distinct"]) == (k, col.n, col.n_strings, e.n_distinct), i
    assert (i["n_nodes"], i["n_edges"], i["n_half_edges"], i["n_hairpins"]) == (n, e.n_edges, m, e.n_hairpins), (i, n, m)
    assert (i["n_rigid"], i["n_palindromes"]) == (sum(e.rigid), sum(e.pal)), i
    assert (i["n_unitigs"], i["n_circular"], i["n_cells"]) == (u, int(e.circular.sum()), len(e.cells)), (i, u)
    assert i["longest_unitig"] == max([len(p) for p in e.unitigs] + [0]), i
    assert i["jump_rounds"] <= 2 * (max(2 * n - 1, 0).bit_length() + 1), i
    assert i["edge_backward_steps"] % 2 == 0 and i["edge_backward_steps"] >= 2 * n and i["mate_backward_steps"] <= i["forward_steps"], i
    assert i["handle_bytes"] >= 4 * (6 * n + 4 * m) and (i["scratch_bytes"] >= col.n // 2 or col.n == 0), i
    assert i["cells_forward_steps"] >= n, i
    invariants(i, o)
    if n:                                                                      # the node table is canonical_kmers' with the same arguments
        lo, count, mate_lo, total, cells = fm.canonical_kmers(k, min_count, max_count, pairs=pairs, cell_bytes=8)
        for name, want in (("lo", lo), ("count", count), ("mate_lo", mate_lo), ("total", total)):
            assert np.array_equal(o[name], want), name
        assert [tuple(int(v) for v in row) for row in cells] == e.keys
    assert [int(v) for v in o["count"]] == e.count and [int(v) for v in o["total"]] == e.total
    assert [int(a) == int(b) for a, b in zip(o["mate_lo"], o["lo"])] == e.pal
    assert [int(a) == NONE for a in o["mate_lo"]] == [x is None for x in e.mate]
    want_deg = e.deg.reshape(-1, 2) if n else np.zeros((0, 2), dtype=np.int64)
    for name, want in (("degree0", want_deg[:, 0]), ("degree1", want_deg[:, 1]), ("end_offsets", e.end_offsets),
                       ("other", np.array([b for _, b in e.links], dtype=np.uint64)),
                       ("weight", np.array([e.H[x][0] for x in e.links], dtype=np.uint64)),
                       ("unitig", e.unitig_of), ("rank", e.rank_of), ("orient", e.orient_of), ("node_offsets", e.node_offsets),
                       ("unitig_weight", e.unitig_weight), ("circular", e.circular), ("cells", e.cells.astype(DT[w]))):
        assert np.array_equal(o[name].astype(np.int64), np.asarray(want).astype(np.int64)), (name, k, min_count, max_count, o[name][:8], want[:8])
    assert [int(v) for v in o["nodes"]] == [y for p in e.unitigs for y in p]
    if m:                                                                      # what grlbwt_fm_count answers for the half-edges' windows
        pats = [e.window(a, b) for a, b in e.links]                            # (None: read that way it holds a cell without a complement)
        idx = [j for j, p in enumerate(pats) if p is not None and fc.fits(p, col.w)]
        got = fc.count(fm, mem, [list(pats[j]) for j in idx], col.w)
        for j, (a, b) in zip(idx, got):
            r, c = int(o["fwd_row"][j]), int(o["fwd_count"][j])
            assert (a, b) == (r, r + c) if c else (a == b and r == NONE), (j, a, b, r, c)
        counted = set(idx)
        assert all(int(o["fwd_count"][j]) == 0 for j in range(m) if j not in counted)
        assert [int(c) > 0 for c in o["fwd_count"]] == [e.H[x][1] is not None for x in e.links]
    return i, o, e


# ------------------------------------------------------------------ the cases
def reads_coll(key, want, k, seed, both=False):
    """reads of 50 cells cut to the shortest prefix with exactly `want` classes of k cells (a further cell adds at most one);
    both: every read's reverse complement too, which adds no class"""
    def make():
        rng = np.random.default_rng(seed)
        flat = mc.ACGT[rng.integers(0, 4, size=2 * want + 200)]
        seen, out, classes = set(), [], 0
        for j0 in range(0, len(flat), 50):
            cur = []
            for c in flat[j0:j0 + 50]:
                cur.append(int(c))
                x = tuple(cur[-k:])
                if len(x) == k and x not in seen:
                    seen |= {x, tuple(int(v) for v in revcomp(np.array(x)))}
                    classes += 1
                if classes == want:
                    break
            out.append(np.array(cur, dtype=np.uint8))
            if classes == want:
                break
        assert classes == want
        return mc.text(out + ([revcomp(s) for s in out] if both else []), 10, 1), 1
    return coll_of(key, make)


def run_nodes_around_the_tile(ctx, flags, mem, lib, name):
    """tile_nodes - 1, tile_nodes, tile_nodes + 1 and 3 tile_nodes + 17 classes at k = 11, one strand; the tile itself also with both
    strands, where every node has two heads"""
    TN = tiles(ctx, mem, lib, flags)[0]
    want = target(name, TN)
    col = reads_coll(("cnodes", TN, name), want, 11, 20261101 + want)
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, _, e = check(fm, mem, col, 11)
        assert i["n_nodes"] == want
    if name == "tile":
        col = reads_coll(("cnodes2", TN, name), want, 11, 20261102 + want, both=True)
        with open_coll(ctx, flags, mem, lib, col) as fm:
            i, o, e = check(fm, mem, col, 11)
            assert i["n_nodes"] == want and int(np.count_nonzero(o["mate_lo"] != NONE)) == want
            assert check(fm, mem, col, 11, 3)[0]["n_nodes"] < want


def alternating(L, read, stride, seed):
    """reads of one random genome of L cells, every other read from the reverse strand"""
    rng = np.random.default_rng(seed)
    genome = mc.ACGT[rng.integers(0, 4, size=L)]
    starts = list(range(0, L - read, stride)) + [L - read]
    return genome, [genome[s:s + read] if j % 2 == 0 else revcomp(genome[s:s + read]) for j, s in enumerate(starts)]


def run_cells_around_the_tile(ctx, flags, mem, lib, name, k=20):
    """one random string of tile_cells - 1 .. 3 tile_cells + 17 cells whose k-mers are all different and have no mate: one unitig of
    that many cells.  The same genome as reads from alternating strands: one unitig that mixes + and - nodes, with and without
    mates, whose cells are the genome or its reverse complement"""
    TC = tiles(ctx, mem, lib, flags)[1]
    L = target(name, TC)
    col = coll_of(("ccells", TC, name), lambda: (mc.text([alternating(L, 60, 30, 20261103 + L)[0]], 10, 1), 1))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, e = check(fm, mem, col, k)
        assert (i["n_unitigs"], i["n_cells"], i["n_circular"], i["n_rigid"]) == (1, L, 0, 0), i
        assert i["jump_rounds"] >= 2, i
        assert np.array_equal(o["cells"], col.cells[:-1]) or np.array_equal(o["cells"], revcomp(col.cells[:-1]))
    genome, reads = alternating(L, 60, 30, 20261103 + L)
    col = coll_of(("ccells_alt", TC, name), lambda: (mc.text(reads, 10, 1), 1))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, e = check(fm, mem, col, k)
        assert (i["n_unitigs"], i["n_cells"], i["n_circular"]) == (1, L, 0), i
        minus = o["orient"] == 1
        assert int(np.count_nonzero(minus & (o["mate_lo"] == NONE))) > 10 and int(np.count_nonzero(minus & (o["mate_lo"] != NONE))) > 10
        assert int(np.count_nonzero(~minus)) > 10
        assert np.array_equal(o["cells"], genome) or np.array_equal(o["cells"], revcomp(genome))
        assert i["cells_forward_steps"] >= i["n_nodes"] + (k - 1) * int(np.count_nonzero(minus & (o["mate_lo"] == NONE)))
        with fm.de_bruijn(k) as plain:                                          # the plain graph is split where the coverage changes strand
            assert plain.info()["n_unitigs"] > 2


def run_strands(ctx, flags, mem, lib):
    """a one-strand read set, and the same reads with their reverse complements: at odd k, where the model shows no palindrome and
    no hairpin, the plain graph has exactly twice the unitigs, each the cells of a canonical unitig or their reverse complement"""
    def reads():
        rng = np.random.default_rng(20261104)
        genome = mc.ACGT[rng.integers(0, 4, size=1500)]
        out = [genome[s:s + 40].copy() for s in rng.integers(0, 1500 - 40 + 1, size=300)]
        for j in range(0, len(out), 9):                                         # a substituted cell now and then: branches
            out[j][20] = mc.ACGT[(int(np.flatnonzero(mc.ACGT == out[j][20])[0]) + 1) % 4]
        return out
    one = coll_of("c_one_strand", lambda: (mc.text(reads(), 10, 1), 1))
    both = coll_of("c_both_strands", lambda: (mc.text(reads() + [revcomp(s) for s in reads()], 10, 1), 1))
    k = 15
    with open_coll(ctx, flags, mem, lib, one) as fm:
        i1, _, e1 = check(fm, mem, one, k)
        check(fm, mem, one, k, 2)
    with open_coll(ctx, flags, mem, lib, both) as fm:
        i2, o, e2 = check(fm, mem, both, k)
        assert e2.n == e1.n and e2.n_edges == e1.n_edges and len(e2.unitigs) == len(e1.unitigs) and i2["max_end_degree"] >= 2
        assert not any(e2.pal) and e2.n_hairpins == 0 and all(x is not None for x in e2.mate)
        with fm.de_bruijn(k) as plain:
            pi, un = plain.info(), plain.unitigs()
        assert pi["n_unitigs"] == 2 * i2["n_unitigs"] and pi["n_nodes"] == 2 * i2["n_nodes"]
        off = o["node_offsets"] + np.arange(len(o["node_offsets"]), dtype=np.uint64) * np.uint64(k - 1)
        have = set()
        for j in range(i2["n_unitigs"]):
            c = o["cells"][int(off[j]):int(off[j + 1])]
            have |= {c.tobytes(), revcomp(c).tobytes()}
        po = un["cell_offsets"]
        assert all(un["cells"][int(po[j]):int(po[j + 1])].astype(np.uint8).tobytes() in have for j in range(pi["n_unitigs"]))


def run_all_rigid(ctx, flags, mem, lib):
    """pairs over values the image does not hold: every node is rigid, a unitig of its own, and the links are the plain graph's edges"""
    col = coll_of("reads_small", lambda: text(["ACGTACGGTTACGTAGGT", "TTACGGATTACCGA", "ACGTACG", "GGTTACGTAG"]))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        for k in (2, 3):
            i, o, e = check(fm, mem, col, k, pairs=((1, 2), (3, 3)))
            assert i["n_rigid"] == i["n_unitigs"] == i["n_nodes"] > 3 and i["n_hairpins"] == 0 and bool(np.all(o["orient"] == 0))
            with fm.de_bruijn(k) as plain:
                off, frm, wt, row = plain.edges()
                assert plain.info()["n_nodes"] == i["n_nodes"] and 2 * len(frm) == i["n_half_edges"]
            eo = o["end_offsets"]
            src = np.repeat(np.arange(2 * i["n_nodes"]), np.diff(eo.astype(np.int64)))
            fwd = {(int(a), int(b)): (int(r), int(c), int(x)) for a, b, r, c, x in zip(src, o["other"], o["fwd_row"], o["fwd_count"], o["weight"])}
            for v in range(i["n_nodes"]):
                for j in range(int(off[v]), int(off[v + 1])):
                    assert fwd[(2 * int(frm[j]) + 1, 2 * v)] == (int(row[j]), int(wt[j]), int(wt[j]))


def run_shapes(ctx, flags, mem, lib):
    """the small shapes of the contract, each pinned by hand beside the model"""
    NN = ((65, 84), (67, 71), (78, 78))
    with open_coll(ctx, flags, mem, lib, coll_of("c_acgt", lambda: text(["ACGT"]))) as fm:             # a hairpin
        i, o, _ = check(fm, mem, coll_of("c_acgt", None), 3)
        assert (i["n_nodes"], i["n_edges"], i["n_half_edges"], i["n_hairpins"], i["n_unitigs"]) == (1, 1, 1, 1, 1), i
        assert [int(v) for v in o["other"]] == [1] and int(o["degree1"][0]) == 1 and int(o["weight"][0]) == int(o["fwd_count"][0]) == 1
        i, _, _ = check(fm, mem, coll_of("c_acgt", None), 4)                                          # a palindrome alone
        assert (i["n_nodes"], i["n_palindromes"], i["n_rigid"], i["n_edges"]) == (1, 1, 1, 0), i
        i, _, _ = check(fm, mem, coll_of("c_acgt", None), 2)                                          # AC/GT and the palindrome CG
        assert (i["n_nodes"], i["n_palindromes"]) == (2, 1), i
    col = coll_of("c_pal", lambda: text(["ACGTACGTAATTGAATTCA", "TTANTAANNNCANTG", "GAATTCAATT"]))      # palindromes at even k, and with (N,N)
    with open_coll(ctx, flags, mem, lib, col) as fm:
        for k, pairs in ((2, None), (4, None), (6, None), (2, NN), (3, NN), (4, NN), (5, NN)):
            i, o, e = check(fm, mem, col, k, pairs=pairs)
            assert (i["n_palindromes"] > 0) == (k % 2 == 0 or pairs is NN), (k, i)
            assert bool(np.all(o["degree1"][o["mate_lo"] == o["lo"]] == 0))
        assert check(fm, mem, col, 2, pairs=NN)[0]["n_hairpins"] >= 1                                  # NNN at the palindrome NN
        i, o, e = check(fm, mem, col, 3)                                                              # N without a complement: rigid nodes
        assert i["n_rigid"] > i["n_palindromes"] == 0 and i["n_unitigs"] < i["n_nodes"]
    col = coll_of("c_n", lambda: text(["ACCGATNTTGCAGA", "GGATCTNAACCT"]))                              # beside compactable neighbours
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, e = check(fm, mem, col, 3)
        assert i["n_rigid"] == 6 and i["n_palindromes"] == 0 and i["n_unitigs"] < i["n_nodes"], i      # ATN TNT NTT, CTN TNA NAA
        check(fm, mem, col, 3, pairs=NN)
    for key, strs in (("c_loop1", ["AAAA"]), ("c_loop2", ["AAAA", "TTTT"])):                           # a self-loop, one strand and both
        col = coll_of(key, lambda: text(strs))
        with open_coll(ctx, flags, mem, lib, col) as fm:
            i, o, _ = check(fm, mem, col, 2)
            assert (i["n_nodes"], i["n_edges"], i["n_half_edges"], i["n_unitigs"], i["n_circular"], i["n_hairpins"]) == (1, 1, 2, 1, 1, 0), i
            assert [int(v) for v in o["other"]] == [1, 0] and int(o["weight"][0]) == 2 * len(strs)
            assert [int(c) > 0 for c in o["fwd_count"]] == [len(strs) == 2, True]
    col = coll_of("c_cycle3", lambda: text(["CGTCGTCGTCG", "ACG"]))      # a cycle of 3 nodes; its smallest node {ACG, CGT} is met as the mate
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, e = check(fm, mem, col, 3)
        assert (i["n_nodes"], i["n_unitigs"], i["n_circular"], i["longest_unitig"]) == (3, 1, 1, 3), i
        assert e.keys[0] == (65, 67, 71) and e.mate[0] == (67, 71, 84) and int(o["nodes"][0]) == 0
        assert bytes(o["cells"].astype(np.uint8)) == b"ACGAC"
    col = coll_of("c_cycle2", lambda: text(["GTGTGTG", "ACA"]))          # two nodes joined through ends (0, 0) and (1, 1)
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, e = check(fm, mem, col, 3)
        assert (i["n_nodes"], i["n_unitigs"], i["n_circular"]) == (2, 1, 1), i
        assert sorted(e.links) == [(0, 2), (1, 3), (2, 0), (3, 1)] and [int(v) for v in o["nodes"]] == [0, 3]
    long_cycle = coll_of("c_long_cycle", lambda: (mc.text([np.tile(mc.ACGT[np.random.default_rng(20261105).integers(0, 4, size=301)], 3)], 10, 1), 1))
    with open_coll(ctx, flags, mem, lib, long_cycle) as fm:
        i, _, _ = check(fm, mem, long_cycle, 12)
        assert (i["n_nodes"], i["n_unitigs"], i["n_circular"]) == (301, 1, 1) and i["jump_rounds"] > 10, i
    for key, strs, ks in (("fork", ["ACGTACCA", "ACGTAGGT"], (2, 3, 4)), ("join", ["CCATTGCA", "GGTTTGCA"], (2, 3, 4)),
                          ("bubble", ["ACGTTCATGGA", "ACGTTGATGGA"], (2, 3, 4, 5)), ("c_fork_rc", ["ACGTACCA", "ACCTACGT"], (3, 4))):
        col = coll_of(key, lambda: text(strs))
        with open_coll(ctx, flags, mem, lib, col) as fm:
            for k in ks:
                i, _, _ = check(fm, mem, col, k)
            assert i["max_end_degree"] >= 2 and i["n_unitigs"] > 1
    col = coll_of("c_by_mate", lambda: text(["CCAACTT", "AAGTTGG", "CCAAC"]))
    with open_coll(ctx, flags, mem, lib, col) as fm:                     # classes that pass min_count only through their mates
        i1, _, e1 = check(fm, mem, col, 4)
        i2, o, e2 = check(fm, mem, col, 4, 2)
        assert i2["n_nodes"] == i1["n_nodes"] and any(c < 2 <= t for c, t in zip(e2.count, e2.total))
        assert check(fm, mem, col, 4, 3)[0]["n_nodes"] < i1["n_nodes"]
        i, _, _ = check(fm, mem, col, 4, 1, 2)
        assert 0 < i["n_nodes"] < i1["n_nodes"]
        for mn, mx in ((4, 0), (7, 9)):                                   # every node filtered out: an empty graph
            i, _, _ = check(fm, mem, col, 4, mn, mx)
            assert (i["n_nodes"], i["n_edges"], i["n_unitigs"], i["n_cells"]) == (0, 0, 0, 0) and i["n_distinct"] > 0


def run_values_of_k(ctx, flags, mem, lib):
    col = coll_of("values_of_k", lambda: text(["ACGTACGGT", "ACGT", "", "TTGACGTAC"]))
    with open_coll(ctx, flags, mem, lib, col) as fm:
        check(fm, mem, col, 1)
        check(fm, mem, col, 2)
        i, _, _ = check(fm, mem, col, col.longest)
        assert i["n_nodes"] >= 1 and i["n_edges"] == 0
        for k in (col.longest + 1, 10 ** 6, 2 ** 63):
            i, _, _ = check(fm, mem, col, k)
            assert (i["n_nodes"], i["n_cells"], i["n_distinct"], i["n_half_edges"]) == (0, 0, 0, 0)
    for name in ("one_empty_string", "empty_strings"):                          # no rows with a cell: legal empty graphs
        c = lc.cases(dc.tiles(ctx, mem, lib, flags)[0])[name]
        col = coll_of(("c_small", name), lambda: (c.cells, c.w))
        with open_coll(ctx, flags, mem, lib, col) as fm:
            assert check(fm, mem, col, 1)[0]["n_nodes"] == 0


def run_other_alphabets(ctx, flags, mem, lib, name):
    """caller pairs over the values of a two-byte and of a compacted 64-bit alphabet"""
    c = lc.cases(dc.tiles(ctx, mem, lib, flags)[0])[name]
    col = coll_of(("c_small", name), lambda: (c.cells, c.w))
    v = [int(a) for a in col.vals[1:]]
    assert len(v) >= 6
    absent = max(v) + 5 if max(v) < 2 ** 63 else 7
    assert absent not in v and absent != int(col.vals[0])
    maps = [((v[0], v[1]), (v[2], v[2]), (v[-1], v[3])), tuple(zip(v[0::2], v[1::2]))[:100] + ((absent, absent + 1),), ((v[0], absent),), ()]
    with open_coll(ctx, flags, mem, lib, col) as fm:
        for pairs in maps:
            for k in (1, 2, 3):
                i, o, e = check(fm, mem, col, k, pairs=pairs, w=8)
        assert i["n_rigid"] == i["n_nodes"]                                     # the empty map
        i, o, e = check(fm, mem, col, 1, pairs=maps[0], w=8)
        assert i["n_nodes"] > i["n_rigid"] >= i["n_palindromes"] == 1
        if name == "wide_u64":                                                  # values as values; a narrower width is refused, nothing written
            assert max(v) == 2 ** 63 + 11
            with fm.de_bruijn_canonical(2, pairs=maps[0]) as g:
                i = g.info()
                for w in (1, 2, 4):
                    buf, p = mem.out(i["n_cells"] * w)
                    msg = fc.einval(lambda: g.unitigs_raw(fm, w, cells_ptr=p, capacity_cells=i["n_cells"]))
                    assert "does not fit" in msg and bool(np.all(mem.get(buf) == FILL))
                assert len(g.nodes()["lo"]) == i["n_nodes"] and len(g.links()[1]) == i["n_half_edges"]
    # a - node without a mate is written through the complement's value, which the image does not hold and which must fit
    col = coll_of("c_absent_comp", lambda: text(["CCA"]))                       # CC -> CA, read from the smaller node CA: (300, G, G)
    with open_coll(ctx, flags, mem, lib, col) as fm:
        i, o, e = check(fm, mem, col, 2, pairs=((65, 300), (67, 71)), w=2)
        assert int(np.count_nonzero((o["orient"] == 1) & (o["mate_lo"] == NONE))) >= 1 and 300 in [int(x) for x in o["cells"]]
        with fm.de_bruijn_canonical(2, pairs=((65, 300), (67, 71))) as g:
            buf, p = mem.out(i["n_cells"])
            msg = fc.einval(lambda: g.unitigs_raw(fm, 1, cells_ptr=p, capacity_cells=i["n_cells"]))
            assert "does not fit" in msg and bool(np.all(mem.get(buf) == FILL))


def run_outputs_and_sizing(ctx, flags, mem, lib):
    """every array of every writer alone; each capacity one short is EINVAL with all guards intact; the array-returning forms"""
    col = coll_of("reads_small", lambda: text(["ACGTACGGTTACGTAGGT", "TTACGGATTACCGA", "ACGTACG", "GGTTACGTAG"]))
    L = ctx.L
    with open_coll(ctx, flags, mem, lib, col) as fm:
        _, o, e = check(fm, mem, col, 3)
        with fm.de_bruijn_canonical(3) as g:
            i = g.info()
            n, m, u, nc = i["n_nodes"], i["n_half_edges"], i["n_unitigs"], i["n_cells"]
            assert n > 3 and m > 3 and u > 1
            calls = [
                (lambda p, c: g.nodes_raw(*p, capacity=c[0]), [(name, b * n) for name, b in NODE_COLS], [n], lambda j: 0),
                (lambda p, c: g.links_raw(*p, capacity=c[0]), [("end_offsets", 8 * (2 * n + 1))] + [(x, 8 * m) for x in LINK_COLS[1:]], [m], lambda j: 0),
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
                    assert mem.body(buf, nbytes).tobytes() == o[name].tobytes(), name
                    buf, ptr = mem.out(nbytes)                                   # its capacity one short
                    args = [ptr if x == j else None for x in range(len(arrays))]
                    short = [c - 1 if x == cap_of(j) else c for x, c in enumerate(caps)]
                    msg = fc.einval(lambda: fn(args, short))
                    assert "GRLBWT" not in msg and bool(np.all(mem.get(buf) == FILL)), name
            assert L.grlbwt_cdebruijn_nodes(ctx._h, None, None, None, None, None, None, None, None, None, None, 0) == EINVAL
            nodes, links, un = g.nodes(), g.links(), g.unitigs()
            for name, _ in NODE_COLS:
                assert np.array_equal(nodes[name], o[name]) and nodes[name].dtype == o[name].dtype, name
            assert all(np.array_equal(a, o[b]) for a, b in zip(links, LINK_COLS))
            assert np.array_equal(un["node_offsets"], o["node_offsets"]) and np.array_equal(un["nodes"], o["nodes"])
            assert np.array_equal(un["weight"], o["unitig_weight"]) and np.array_equal(un["circular"], o["circular"])
            assert un["cells"].dtype == np.uint8 and np.array_equal(un["cells"], o["cells"])
            assert np.array_equal(un["cell_offsets"], o["node_offsets"] + np.arange(u + 1, dtype=np.uint64) * np.uint64(2))
            assert "cells" not in g.unitigs(cells=False)


def run_refusals(ctx, flags, mem, lib):
    col = coll_of("reads_small", lambda: text(["ACGTACGGTTACGTAGGT", "TTACGGATTACCGA", "ACGTACG", "GGTTACGTAG"]))
    other = coll_of("other", lambda: text(["GGTTACGTAG", "ACGTACGGTTACGTAGGT", "ACGTACG", "TTACGGATTACCGA"]))
    L = ctx.L
    with open_coll(ctx, flags, mem, lib, col) as fm:
        fc.einval(lambda: fm.de_bruijn_canonical(0))                            # those of grlbwt_debruijn_create
        fc.einval(lambda: fm.de_bruijn_canonical(3, 5, 4))
        fc.einval(lambda: engine.CanonicalDeBruijn(fm, 3, flags=1))
        fm.de_bruijn_canonical(3, 5, 0).close()
        h = C.c_void_p(7)
        assert L.grlbwt_cdebruijn_create(ctx._h, None, 3, 1, 0, None, 0, 0, C.byref(h)) == EINVAL and not h.value
        assert L.grlbwt_cdebruijn_create(ctx._h, fm._h, 3, 1, 0, None, 0, 0, None) == EINVAL
        assert L.grlbwt_cdebruijn_info_get(None, None) == EINVAL
        assert L.grlbwt_cdebruijn_destroy(ctx._h, None) == 0
        many = (C.c_uint64 * 258)(*range(1000, 1258))                           # those of the pairs
        assert L.grlbwt_cdebruijn_create(ctx._h, fm._h, 3, 1, 0, C.cast(many, C.c_void_p), 129, 0, C.byref(h)) == EINVAL and not h.value
        assert "129" in L.grlbwt_last_error(ctx._h).decode()
        assert L.grlbwt_cdebruijn_create(ctx._h, fm._h, 3, 1, 0, None, 3, 0, C.byref(h)) == EINVAL and "NULL" in L.grlbwt_last_error(ctx._h).decode()
        for pairs, bad in ((((65, 84), (65, 71)), 65), (((65, 84), (84, 65)), 65), (((67, 67), (67, 71)), 67), (((65, 84), (10, 71)), 10), (((10, 10),), 10)):
            msg = fc.einval(lambda: fm.de_bruijn_canonical(3, pairs=pairs))
            assert str(bad) in msg and ("separator" in msg) == (bad == 10), (pairs, msg)
        fm.de_bruijn_canonical(3, pairs=[(1000 + 2 * i, 1001 + 2 * i) for i in range(128)]).close()      # (legal: 128 pairs)
        with fm.de_bruijn_canonical(3) as g, open_coll(ctx, flags, mem, lib, other) as fm2:
            i = g.info()
            buf, ptr = mem.out(i["n_cells"])
            msg = fc.einval(lambda: g.unitigs_raw(fm2, 1, cells_ptr=ptr, capacity_cells=i["n_cells"]))          # a second index
            assert "not the index" in msg and "GRLBWT" not in msg and bool(np.all(mem.get(buf) == FILL))
            fc.einval(lambda: g.unitigs_raw(None, 1, cells_ptr=ptr, capacity_cells=i["n_cells"]))               # the cells without an index
            for w in (0, 3, 16):
                fc.einval(lambda: g.unitigs_raw(fm, w, cells_ptr=ptr, capacity_cells=i["n_cells"]))
            fc.einval(lambda: g.nodes_raw(lo_ptr=ptr + 4, capacity=i["n_nodes"]))                               # not aligned
            assert bool(np.all(mem.get(buf) == FILL))
            g.unitigs_raw(fm, 1, cells_ptr=ptr, capacity_cells=i["n_cells"])
            mem.body(buf, i["n_cells"])
            with fm.de_bruijn(3) as plain:                                      # the two kinds of handle do not mix
                assert L.grlbwt_cdebruijn_destroy(ctx._h, plain._h) == EINVAL
    bad = ic.make_image(1, 1, [10, 65], [1, 2])              # not the BWT of a collection: the row of the second A is LF of itself
    keep, img = mem.put(bad)
    with engine.FmIndex(ctx, img, len(bad)) as fm:
        msg = fc.einval(lambda: fm.de_bruijn_canonical(3))
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
        fm.canonical_kmers(4)                                                   # an earlier call: its counters stay
        before, counts = fm.info(), fc.count(fm, mem, pats, 1)
        check(fm, mem, c, 3)
        cinfo, kinfo = fm.canonical_kmer_info(), fm.kmer_info()                 # (check's own canonical_kmers wrote the first)
        with fm.de_bruijn_canonical(7, 2) as g:
            assert fm.info() == before and fm.canonical_kmer_info() == cinfo and fm.kmer_info() == kinfo, kw
        _, o, _ = check(fm, mem, c, 7, 2)                                       # (check itself calls canonical_kmers)
        assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts, kw
        g = fm.de_bruijn_canonical(7, 2)
        fm.close()                                                              # the handle survives its index
        nodes, links = g.nodes(), g.links()
        assert np.array_equal(nodes["lo"], o["lo"]) and np.array_equal(nodes["unitig"], o["unitig"]) and np.array_equal(nodes["orient"], o["orient"])
        assert all(np.array_equal(a, o[b]) for a, b in zip(links, LINK_COLS))
        assert np.array_equal(g.unitigs(cells=False)["nodes"], o["nodes"])
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
        vals = sorted(set(int(v) for v in c.syms)) if hasattr(c, "syms") else []
        for k in (1, 2, 5):
            for pairs in (None, tuple((a, b) for a, b in zip(vals[1::2], vals[2::2]))[:128])[:2 if k == 2 else 1]:
                try:
                    g = fm.de_bruijn_canonical(k, pairs=pairs)
                except engine.GrlbwtError as e:
                    assert e.code == EINVAL, e
                    refused += 1
                    continue
                with g:
                    i, o = read_all(g, fm, mem, 8)
                    assert i["n_nodes"] <= n and i["n_half_edges"] <= 2 * n and i["n_nodes"] == fm.canonical_kmers_raw(k, pairs=pairs)
                    invariants(i, o)
                    assert bool(np.all(o["lo"][1:] > o["lo"][:-1])) and bool(np.all(o["lo"] + o["count"] <= n))
                    assert bool(np.all(o["fwd_row"][o["fwd_count"] > 0] + o["fwd_count"][o["fwd_count"] > 0] <= n))
                done += 1
    return done, refused
