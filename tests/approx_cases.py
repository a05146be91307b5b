"""Shared by tests/test_fm_approx_sim.py (serial stand-in) and tests/test_fm_approx_gpu.py (HIP library): every occurrence of a
pattern with up to k substituted cells (grlbwt_fm_approx), against values from code that shares nothing with the engine.

  A  collections the engine builds (fm_cases.COLS): the hits BY DEFINITION ON THE TEXT -- the distinct separator-free windows
     within Hamming distance k of the pattern -- their rows from fm_cases.count of each variant (tested elsewhere against the
     text), their order from the header's rule as a sort key, sub_pos / sub_val must rebuild the variant.
  B  the pattern set is not vacuous (on the brute-force values only).
  C  foreign images (tests/image_cases.py): a recursive search in Python on the RECORDS (fm_cases.RecordIndex).
  D  launch shapes: 0, 1, 63, 64, 65 and 5000 patterns of 6 to 10 cells at k = 1, empty ones between them, off[0] = 7.
  E  max_hits: each list is the head of the full one, n_truncated the number of lists that were longer.
  F  refusals and the sizing call.

Every output buffer has guard bytes behind it (fm_cases.Mem); the info of every call is checked against its outputs.  The
brute-force values are computed once per process and kept.

COST, and what it means here.  A cell at which a substitution is open costs sigma - 2 backward steps, so at k = 2 ANY pattern of
two cells or more costs about sigma^2 dependent steps of ONE lane: a million for `two_bytes` (sigma 983), seconds on a GPU lane
whatever the number of patterns.  `two_bytes` therefore runs k = 2 on a subset: the patterns of at most one cell (the special
ones among them) everywhere, and on the serial stand-in, whose steps are cheap, also one substring with a changed cell and one
random pattern of two cells.  Every other collection runs every pattern at every k.
"""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import match_cases as mc

DT = fc.DT
NONE = fc.NONE
K_MAX = {"dna": 3, "single": 3, "identical": 3, "two_bytes": 2, "wide_u64": 2}
SHAPES = (0, 1, 63, 64, 65, 5000)
SEED = 20261019
HEAVY_SIGMA = 64           # above: the k = 2 subset of the module comment


# ------------------------------------------------------------------ the call on a batch, guarded outputs, info checked
def sizing(fm, pc, w, po, n, k, max_hits):
    """the sizing call: capacity 0 and no arrays; -> the number of hits"""
    try:
        return fm.approx(pc, w, po, n, k, max_hits, None, None, None, None, 0)
    except engine.GrlbwtError as e:
        assert e.code == fc.EINVAL, e
        return e.n_hits


def approx(fm, mem, patterns, w, k, max_hits=0, subs=True, lead=0, capacity=None, n_truncated=None):
    """grlbwt_fm_approx on a batch -> per pattern the list of (substitutions, lo, hi, ((offset, value), ...)) in the order written
    (the last member None without the sub arrays); the info of the call.  capacity None: what the sizing call reports."""
    keep, pc, po, nc = mc.put_batch(mem, patterns, w, lead)
    n = len(patterns)
    cap = sizing(fm, pc, w, po, n, k, max_hits) if capacity is None else capacity
    hoff, ph = mem.out(8 * (n + 1))
    cols = [mem.out(8 * cap) for _ in range(3)]
    sp, psp = mem.out(8 * cap * k)
    sv, psv = mem.out(8 * cap * k)
    got = fm.approx(pc, w, po, n, k, max_hits, ph, cols[0][1], cols[1][1], cols[2][1], cap, psp if subs else None, psv if subs else None)
    assert got <= cap
    H = mem.body(hoff, 8 * (n + 1)).view(np.uint64)
    assert int(H[0]) == 0 and int(H[-1]) == got and bool(np.all(H[1:] >= H[:-1])), H[:8]
    for b, _ in cols:
        assert bool(np.all(mem.get(b)[8 * got:] == fc.FILL)), "entries behind the last one were written"
    mism, lo, hi = [mem.body(b, 8 * cap).view(np.uint64)[:got] for b, _ in cols]
    if subs:
        assert bool(np.all(mem.get(sp)[8 * got * k:] == fc.FILL)) and bool(np.all(mem.get(sv)[8 * got * k:] == fc.FILL))
        P = mem.body(sp, 8 * cap * k).view(np.uint64)[:got * k].reshape(got, k)
        V = mem.body(sv, 8 * cap * k).view(np.uint64)[:got * k].reshape(got, k)
    else:
        assert bool(np.all(mem.get(sp) == fc.FILL)) and bool(np.all(mem.get(sv) == fc.FILL))
    out = []
    for i in range(n):
        hits = []
        for j in range(int(H[i]), int(H[i + 1])):
            d = int(mism[j])
            assert d <= k
            s = None
            if subs:
                assert bool(np.all(P[j, d:] == np.uint64(NONE))) and bool(np.all(V[j, d:] == np.uint64(NONE))), (i, j)
                s = tuple((int(P[j, t]), int(V[j, t])) for t in range(d))
                assert all(a[0] > b[0] for a, b in zip(s, s[1:])), s
            hits.append((d, int(lo[j]), int(hi[j]), s))
        out.append(hits)
    info = fm.approx_info()
    assert (info["n_patterns"], info["n_cells"], info["max_mismatches"], info["max_hits"]) == (n, nc, k, max_hits), info
    assert info["n_hits"] == got and info["table_bytes"] == 0, info
    assert info["hits_by_mismatches"] == [int((mism == np.uint64(d)).sum()) for d in range(4)], info
    if max_hits:
        assert all(len(h) <= max_hits for h in out)
        assert info["n_truncated"] <= sum(1 for h in out if len(h) == max_hits), info
    else:
        assert info["n_truncated"] == 0, info
    if n_truncated is not None:
        assert info["n_truncated"] == n_truncated, (info, n_truncated)
    if k == 0:
        assert info["steps"] <= nc, info
    assert info["steps"] >= sum(len(p) for p, h in zip(patterns, out) if h), info          # a hit took a step per cell at least
    return out, info


def rebuilt(q, hit):
    """the variant a hit stands for"""
    v = list(q)
    for x, c in hit[3]:
        assert 0 <= x < len(q) and c != q[x], (q, hit)
        v[x] = c
    return v


# ------------------------------------------------------------------ A: by definition, on the text
def order_key(q, v):
    """the header's rule as a sort key: from the last offset down, a cell that differs from the pattern comes before one that
    equals it, and among differing cells the smaller symbol first"""
    return tuple((v[x] == q[x], v[x]) for x in range(len(q) - 1, -1, -1))


def variants(col, q, kmax):
    """(substitutions, variant) of every distinct separator-free window of the text within Hamming distance kmax of q, in the
    order of the rule"""
    m = len(q)
    if m == 0:
        return [(0, [])]
    if m > col.n:
        return []
    win = np.lib.stride_tricks.sliding_window_view(col.data, m)
    is_sep = np.concatenate([[0], np.cumsum(col.data == col.data.dtype.type(col.sep))])
    clean = (is_sep[m:] - is_sep[:-m]) == 0
    dist = (win != np.array(q, dtype=col.data.dtype)).sum(axis=1)
    idx = np.flatnonzero(clean & (dist <= kmax))
    if not len(idx):
        return []
    rows = np.unique(win[idx], axis=0)
    out = []
    for r in rows:
        v = [int(x) for x in r]
        out.append((sum(1 for a, b in zip(v, q) if a != b), v))
    out.sort(key=lambda dv: order_key(q, dv[1]))
    return out


def collection_patterns(col):
    """Substrings of 8 to 32 cells with 0 to 3 cells changed to a body symbol, a non-symbol or the separator; random patterns of
    1, 2, 3, 5 cells; [], one non-symbol, the separator alone, one pattern longer than any string.  144 of them (52 where the
    alphabet is large)."""
    rng = np.random.default_rng(SEED)
    body = sorted(set(int(v) for v in np.unique(col.data)) - {col.sep})
    full = [[int(v) for v in s] for s in col.strings if len(s)]
    longest = max(len(s) for s in full)
    long_enough = [s for s in full if len(s) >= min(8, longest)]
    bad = mc.non_symbol(col)
    pats = []
    for _ in range(28 if len(body) > HEAVY_SIGMA else 120):
        s = long_enough[int(rng.integers(len(long_enough)))]
        m = min(int(rng.integers(8, 33)), len(s))
        a = int(rng.integers(0, len(s) - m + 1))
        q = s[a:a + m]
        for _ in range(int(rng.integers(0, 4))):
            x = int(rng.integers(m))
            kind = rng.random()
            q[x] = bad if kind < 0.1 else col.sep if kind < 0.2 else body[int(rng.integers(len(body)))]
        pats.append(q)
    for m in (1, 2, 3, 5):
        for _ in range(5):
            pats.append([body[int(rng.integers(len(body)))] for _ in range(m)])
    pats += [[], [bad], [col.sep], [body[i % len(body)] for i in range(longest + 3)]]
    return pats


class Expected:
    """per pattern the (substitutions, variant) list at the collection's largest k; the list at a smaller k is its filter"""

    def __init__(self, name):
        self.col = col = fc.COLS[name]
        self.kmax = K_MAX[name]
        self.pats = collection_patterns(col)
        self.heavy = len(np.unique(col.data)) - 1 > HEAVY_SIGMA
        self.var = []
        for i, q in enumerate(self.pats):
            k = self.kmax
            if self.heavy and len(q) > 1 and i not in self.k2_extra():
                k = min(k, 1)
            self.var.append(variants(col, q, k))
        self._rows = {}

    def k2_extra(self):
        """the two longer patterns a large alphabet runs at k = 2 on the stand-in: a substring with a changed cell, two random cells"""
        sub = next(i for i, q in enumerate(self.pats) if len(q) >= 8)
        two = next(i for i, q in enumerate(self.pats) if len(q) == 2)
        return (sub, two)

    def batch(self, k, on_gpu):
        """the indexes of the patterns that run at this k (module comment)"""
        if not (self.heavy and k >= 2):
            return list(range(len(self.pats)))
        return [i for i, q in enumerate(self.pats) if len(q) <= 1 or (not on_gpu and i in self.k2_extra())]

    def lists(self, k, idx):
        return [[(d, v) for d, v in self.var[i] if d <= k] for i in idx]

    def want(self, fm, mem, k, idx):
        """per pattern the expected entries (substitutions, lo, hi, subs); the rows of every variant from fm.count, once per index"""
        key = id(fm)
        if key not in self._rows:
            flat = [v for lst in self.var for _, v in lst if v]
            got = fc.count(fm, mem, flat, self.col.w)
            self._rows = {key: {tuple(v): r for v, r in zip(flat, got)}}
        rows = self._rows[key]
        out = []
        for i, lst in zip(idx, self.lists(k, idx)):
            q = self.pats[i]
            ent = []
            for d, v in lst:
                lo, hi = rows[tuple(v)] if v else (0, self.col.n)
                assert lo < hi, (q, v)
                ent.append((d, lo, hi, tuple((x, v[x]) for x in range(len(q) - 1, -1, -1) if v[x] != q[x])))
            out.append(ent)
        return out


_expected = {}


def expected(name):
    if name not in _expected:
        _expected[name] = Expected(name)
    return _expected[name]


def not_vacuous(ex):
    """B, for the DNA collection, on the text alone.  (The seed gives, at k = 1, 2, 3: the figures of the docstring of
    test_pattern_set_is_not_vacuous.)"""
    per = {k: [len(l) for l in ex.lists(k, range(len(ex.pats)))] for k in (1, 2, 3)}
    assert sum(1 for n in per[1] if n >= 2) >= 12, per[1]
    assert sum(per[2]) >= 500 and sum(1 for n in per[2] if n == 0) >= 6, (sum(per[2]), per[2])
    assert max(per[3]) >= 64, max(per[3])
    return {k: (sum(v), sum(1 for n in v if n >= 2), sum(1 for n in v if n == 0), max(v)) for k, v in per.items()}


def run_collection(ctx, flags, mem, lib, name):
    """A on one collection at k = 0 .. its largest: entries, order and substitutions; the same without the sub arrays and as
    8-byte cells; at k = 0 against grlbwt_fm_count"""
    ex = expected(name)
    col = ex.col
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        del keep
        before = fm.info()["index_bytes"]
        for k in range(ex.kmax + 1):
            idx = ex.batch(k, mem.on_gpu)
            pats = [ex.pats[i] for i in idx]
            want = ex.want(fm, mem, k, idx)
            total = sum(len(e) for e in want)
            got, info = approx(fm, mem, pats, col.w, k, capacity=total)
            bad = [(i, pats[i][:8], g[:3], e[:3]) for i, (g, e) in enumerate(zip(got, want)) if g != e]
            assert not bad, (name, k, bad[:3])
            for q, hits in zip(pats, got):                          # the substitutions rebuild a variant that differs where they say
                for h in hits:
                    assert len(rebuilt(q, h)) == len(q)
            plain, _ = approx(fm, mem, pats, col.w, k, subs=False, capacity=total)
            assert [[h[:3] for h in hs] for hs in plain] == [[e[:3] for e in es] for es in want], (name, k)
            if col.w < 8 and k <= (0 if ex.heavy else 1):           # the same patterns as wider cells
                wide, _ = approx(fm, mem, pats, 8, k, capacity=total)
                assert wide == got, (name, k)
            if k == 0:
                ok = [i for i, q in enumerate(pats) if col.sep not in q and all(v in set(col.data.tolist()) for v in q)]
                cnt = fc.count(fm, mem, [pats[i] for i in ok], col.w)
                for i, (lo, hi) in zip(ok, cnt):
                    assert [h[1:3] for h in got[i]] == ([(lo, hi)] if lo < hi else []), (name, pats[i][:8])
        assert fm.info()["index_bytes"] == before                 # no table: the index holds what it held


# ------------------------------------------------------------------ C: by definition, on the records of a foreign image
def search_records(ri, q, k):
    """the enumeration of the header on fm_cases.RecordIndex, as a recursion"""
    sep = ri.present[0] if ri.present else None
    body = ri.present[1:]
    out = []

    def step(c, lo, hi):
        return ri.C[c] + ri.rank(c, lo), ri.C[c] + ri.rank(c, hi)

    def rec(x, lo, hi, subs):
        if x == 0:
            out.append((len(subs), lo, hi, tuple(subs)))
            return
        own = q[x - 1]
        if len(subs) < k:
            for c in body:
                if c != own:
                    a, b = step(c, lo, hi)
                    if a < b:
                        rec(x - 1, a, b, subs + [(x - 1, c)])
        if own in ri.per and own != sep:
            a, b = step(own, lo, hi)
            if a < b:
                rec(x - 1, a, b, subs)

    if not q or ri.n:
        rec(len(q), 0, ri.n, [])
    return out


_foreign = {}


def foreign_expected(c):
    if c.name not in _foreign:
        ri = fc.RecordIndex(c.syms, c.lens)
        qs = fc.foreign_patterns(c, ri)
        _foreign[c.name] = (ri, qs, {k: [search_records(ri, q, k) for q in qs] for k in (0, 1, 2)})
    return _foreign[c.name]


def run_foreign(ctx, mem, c):
    ri, qs, want = foreign_expected(c)
    for q, hits in zip(qs, want[0]):                               # at k = 0 the recursion is the whole-pattern search
        sep = ri.present[0] if ri.present else None
        if sep not in q:
            assert [h[1:3] for h in hits] == ([ri.search(q)] if ri.search(q) != (0, 0) or not q else []), q
    blob = c.image()
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        del keep
        for w in (1, 2, 4, 8):
            idx = [i for i, q in enumerate(qs) if fc.fits(q, w)]
            for k in (0, 1, 2):
                got, _ = approx(fm, mem, [qs[i] for i in idx], w, k)
                bad = [(qs[i], g[:3], want[k][i][:3]) for i, g in zip(idx, got) if g != want[k][i]]
                assert not bad, (c.name, w, k, bad[:3])


# ------------------------------------------------------------------ D: launch shapes
_pool = []


def shape_pool():
    """40 patterns of 6 to 10 cells of the DNA collection, half of them with a changed cell, and their lists at k = 1"""
    if not _pool:
        col = fc.COLS["dna"]
        rng = np.random.default_rng(SEED + 1)
        full = [[int(v) for v in s] for s in col.strings if len(s) >= 10]
        pats = []
        for j in range(40):
            s = full[int(rng.integers(len(full)))]
            m = int(rng.integers(6, 11))
            a = int(rng.integers(0, len(s) - m + 1))
            q = s[a:a + m]
            if j % 2:
                x = int(rng.integers(m))
                q[x] = [v for v in (65, 67, 71, 84) if v != q[x]][int(rng.integers(3))]
            pats.append(q)
        _pool.append((pats, [variants(col, q, 1) for q in pats]))
    return _pool[0]


def run_shapes(ctx, flags, mem, lib, on_info=None):
    """every shape: n patterns, every fourth one empty, 7 cells in front of the first; on_info(n, info) sees the launch counters"""
    col = fc.COLS["dna"]
    pool, var = shape_pool()
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        flat = [v for lst in var for _, v in lst]
        rows = {tuple(v): r for v, r in zip(flat, fc.count(fm, mem, flat, 1))}
        ent = [[(d, rows[tuple(v)][0], rows[tuple(v)][1], tuple((x, v[x]) for x in range(len(q) - 1, -1, -1) if v[x] != q[x])) for d, v in lst]
               for q, lst in zip(pool, var)]
        assert sum(1 for e in ent if len(e) >= 2) >= 5 and all(r[0] < r[1] for r in rows.values())
        for n in SHAPES:
            pats, want = [], []
            for i in range(n):
                if i % 4 == 3:
                    pats.append([])
                    want.append([(0, 0, col.n, ())])
                else:
                    pats.append(pool[i % len(pool)])
                    want.append(ent[i % len(pool)])
            got, info = approx(fm, mem, pats, 1, 1, lead=7)
            assert got == want, (n, [i for i, (g, e) in enumerate(zip(got, want)) if g != e][:5])
            if on_info:
                on_info(n, info)


# ------------------------------------------------------------------ E: max_hits
def run_max_hits(ctx, flags, mem, lib):
    ex = expected("dna")
    blob = fc.image_of(lib, ex.col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        idx = list(range(len(ex.pats)))
        full = ex.want(fm, mem, 2, idx)
        for cap in (1, 3):
            longer = sum(1 for e in full if len(e) > cap)
            exact = sum(1 for e in full if len(e) == cap)
            assert longer >= 10 and exact >= 1, (cap, longer, exact)
            got, info = approx(fm, mem, ex.pats, 1, 2, max_hits=cap, n_truncated=longer)
            assert got == [e[:cap] for e in full], cap


# ------------------------------------------------------------------ F: refusals
def run_refusals(ctx, flags, mem, lib):
    ex = expected("dna")
    pats = ex.pats[:40]
    blob = fc.image_of(lib, ex.col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        n = len(pats)
        want = ex.want(fm, mem, 1, list(range(n)))
        total = sum(len(e) for e in want)
        assert total >= 2
        keepb, pc, po, _ = mc.put_batch(mem, pats, 1)
        outs = [mem.out(8 * (n + 1))] + [mem.out(8 * total) for _ in range(5)]
        ptr = [p for _, p in outs]

        def untouched():
            return all(bool(np.all(mem.get(b) == fc.FILL)) for b, _ in outs)

        def call(cells=pc, w=1, off=po, np_=n, k=1, hoff=ptr[0], sp=ptr[4], sv=ptr[5], cap=total):
            return fm.approx(cells, w, off, np_, k, 0, hoff, ptr[1], ptr[2], ptr[3], cap, sp, sv)

        kd, pd = mem.put(np.array([0, 2, 1, 3], dtype=np.uint64).tobytes())
        for bad in (lambda: call(k=4),                               # more than three substitutions
                    lambda: call(w=3), lambda: call(w=0),            # a bad width
                    lambda: call(off=pd, np_=3),                     # decreasing offsets
                    lambda: call(cells=None),                        # cells missing while there are some
                    lambda: call(hoff=None),                         # no hit offsets
                    lambda: call(sv=None), lambda: call(sp=None)):   # one sub array without the other
            fc.einval(bad)
            assert untouched()
        L = ctx.L                                                   # a null index
        got = engine.C.c_uint64(7)
        assert L.grlbwt_fm_approx(ctx._h, None, pc, 1, po, n, 1, 0, ptr[0], ptr[1], ptr[2], ptr[3], None, None, total, engine.C.byref(got)) == fc.EINVAL
        assert got.value == 0
        assert L.grlbwt_fm_approx_info_get(None, None) == fc.EINVAL
        assert untouched()
        # one entry too few: the code, the number, nothing written; the sizing call takes capacity 0 and no arrays
        with pytest.raises(engine.GrlbwtError) as e:
            call(cap=total - 1)
        assert e.value.code == fc.EINVAL and e.value.n_hits == total, (e.value, total)
        assert "GRLBWT" not in str(e.value)
        assert untouched()
        assert sizing(fm, pc, 1, po, n, 1, 0) == total
        assert untouched()
        got, _ = approx(fm, mem, pats, 1, 1)                       # the reported capacity suffices
        assert got == want
        # k = 0 with null sub arrays, and with them: an entry owns no word
        exact = ex.want(fm, mem, 0, list(range(n)))
        got, _ = approx(fm, mem, pats, 1, 0, subs=False)
        assert [[h[:3] for h in hs] for hs in got] == [[x[:3] for x in es] for es in exact]
        got, _ = approx(fm, mem, pats, 1, 0)
        assert got == exact
