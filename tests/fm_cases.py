"""Shared by tests/test_fm_index_sim.py (serial stand-in) and tests/test_fm_index_gpu.py (HIP library): counting and
locating patterns in an .rl_bwt image (grlbwt_fm_*), against values from code that shares nothing with the engine.

  A  foreign images (tests/image_cases.py): the backward search by definition on the RECORDS -- per symbol the cumulative
     lengths of its records and np.searchsorted for rank_c(p) -- so the images with lengths of 2^32 and 2^40 run too.
  B  images the engine builds from small collections: hi - lo against a sliding compare over the text.
  C  locate: the (string, offset) set of every pattern against the positions that compare found; for the DNA collection
     every ROW against the suffixes sorted by Python (content, then the string's number: the BCR order).
  D  launch shapes: 0, 1, 63, 64, 65 and 5000 patterns / rows.
  E  refusals.

Every output buffer has guard bytes behind it.  The images of B are built once per library and kept.
"""
import os
import zlib

import numpy as np
import pytest

from grlbwt_amd import engine
from tests import bcr_check as bc
from tests import image_cases as ic
from tests import wide_check as wc

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -22
GUARD = 64
FILL = 0xA5
NONE = 2 ** 64 - 1
DT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
FOREIGN = [c.name for c in ic.CASES if c.R >= 1]
COLLECTIONS = ["dna", "single", "identical", "two_bytes", "wide_u64"]
SHAPES = (0, 1, 63, 64, 65, 5000)


# ------------------------------------------------------------------ device memory of either entry, guarded outputs
class Mem:
    def __init__(self, on_gpu):
        self.on_gpu = on_gpu
        if on_gpu:
            import torch
            self.torch = torch
            torch.zeros(1, device="cuda:0")      # torch's HIP runtime has to be the one the process initialises first

    def put(self, data):
        a = np.frombuffer(bytes(data), dtype=np.uint8).copy()
        if not len(a):
            a = np.zeros(8, dtype=np.uint8)
        if self.on_gpu:
            t = self.torch.from_numpy(a).to("cuda:0")
            self.torch.cuda.synchronize()
            return t, t.data_ptr()
        return a, a.ctypes.data

    def out(self, nbytes):
        if self.on_gpu:
            t = self.torch.full((nbytes + GUARD,), FILL, dtype=self.torch.uint8, device="cuda:0")
            self.torch.cuda.synchronize()
            return t, t.data_ptr()
        a = np.full(nbytes + GUARD, FILL, dtype=np.uint8)
        return a, a.ctypes.data

    def get(self, buf):
        if self.on_gpu:
            self.torch.cuda.synchronize()
            return buf.cpu().numpy()
        return buf

    def body(self, buf, nbytes):
        h = self.get(buf)
        assert bool(np.all(h[nbytes:] == FILL)), "bytes behind the output were written"
        return h[:nbytes].copy()


def einval(fn):
    with pytest.raises(engine.GrlbwtError) as e:
        fn()
    assert e.value.code == EINVAL, e.value
    return str(e.value)


def pack(patterns, w):
    """patterns (lists of ints) -> (cells of w bytes, uint64 offsets)"""
    off = np.zeros(len(patterns) + 1, dtype=np.uint64)
    if patterns:
        off[1:] = np.cumsum([len(p) for p in patterns], dtype=np.uint64)
    cells = np.array([v for p in patterns for v in p], dtype=DT[w])
    return cells, off


def count(fm, mem, patterns, w):
    """grlbwt_fm_count on a batch: the (lo, hi) pairs"""
    cells, off = pack(patterns, w)
    kc, pc = mem.put(cells.tobytes())
    ko, po = mem.put(off.tobytes())
    n = len(patterns)
    lo, plo = mem.out(8 * n)
    hi, phi = mem.out(8 * n)
    fm.count(pc, w, po, n, plo, phi)
    a, b = mem.body(lo, 8 * n).view(np.uint64), mem.body(hi, 8 * n).view(np.uint64)
    return [(int(x), int(y)) for x, y in zip(a, b)]


def locate(fm, mem, rows, max_steps=NONE):
    rows = np.asarray(rows, dtype=np.uint64)
    kr, pr = mem.put(rows.tobytes())
    n = len(rows)
    s, ps = mem.out(8 * n)
    o, po = mem.out(8 * n)
    fm.locate(pr, n, max_steps, ps, po)
    return mem.body(s, 8 * n).view(np.uint64), mem.body(o, 8 * n).view(np.uint64)


def fits(p, w):
    return all(v < 1 << (8 * w) for v in p)


# ------------------------------------------------------------------ A: by definition, on the records
class RecordIndex:
    """rank_c(p) from the records alone: per symbol the starts of its non-empty records and the lengths in front of them."""

    def __init__(self, syms, lens):
        keep = lens != 0
        syms, lens = syms[keep], lens[keep]
        self.n = int(lens.sum(dtype=np.uint64))
        starts = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)[:-1]]).astype(np.uint64) if len(lens) else lens
        self.present = sorted(int(s) for s in np.unique(syms))
        self.per, self.C = {}, {}
        below = 0
        for c in self.present:
            m = syms == np.uint64(c)
            ln = lens[m]
            self.per[c] = (starts[m], ln, np.concatenate([[0], np.cumsum(ln, dtype=np.uint64)]).astype(np.uint64))
            self.C[c] = below
            below += int(ln.sum(dtype=np.uint64))

    def rank(self, c, p):
        st, ln, cum = self.per[c]
        j = int(np.searchsorted(st, np.uint64(p), side="left"))          # records of c that start before p
        if j == 0:
            return 0
        return int(cum[j - 1]) + min(p - int(st[j - 1]), int(ln[j - 1]))

    def search(self, pattern):
        lo, hi = 0, self.n
        for c in reversed(pattern):
            if lo >= hi or c not in self.per:
                return 0, 0
            lo, hi = self.C[c] + self.rank(c, lo), self.C[c] + self.rank(c, hi)
        return (lo, hi) if lo < hi else (0, 0)


def foreign_patterns(c, ri):
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    present = ri.present
    pats = [[s] for s in present]
    if present:
        sep, body = present[0], present[1:]
        if sep > 0:
            pats.append([sep - 1])
        gaps = [a + 1 for a, b in zip(present, present[1:]) if b - a > 1]
        if gaps:
            pats.append([gaps[len(gaps) // 2]])
        if present[-1] < 2 ** 64 - 1:
            pats.append([present[-1] + 1])
        if c.sb < 8:
            pats.append([1 << (8 * c.sb)])                       # does not fit the image's symbol width
            pats.append([body[0] if body else sep, 1 << (8 * c.sb)][::-1])
        pats += [[a, b] for a in body for b in body]
        for _ in range(200):
            m = int(rng.integers(1, 5)) if body else 1
            p = [body[int(rng.integers(len(body)))] for _ in range(m - 1)] + [present[int(rng.integers(len(present)))]]
            pats.append(p)
    else:
        pats += [[0], [65], [65, 0]]
    pats.append([])
    return pats


def run_foreign(ctx, mem, c):
    """count on a foreign image, every cell width that holds the pattern; then the index with the locate structures is
    either made or refused"""
    ri = RecordIndex(c.syms, c.lens)
    pats = foreign_patterns(c, ri)
    want = [ri.search(p) for p in pats]
    assert want[-1] == ((0, ri.n) if ri.n else (0, 0))
    blob = c.image()
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        del keep                                                  # the index has copied what it needs
        info = fm.info()
        assert (info["n_syms"], info["sigma"], info["flags"]) == (ri.n, len(ri.present), 0)
        assert info["n_runs"] == int((c.lens != 0).sum())
        if ri.present:
            sep = ri.present[0]
            assert info["separator"] == sep and info["n_strings"] == ri.rank(sep, ri.n)
        for w in (1, 2, 4, 8):
            idx = [i for i, p in enumerate(pats) if fits(p, w)]
            got = count(fm, mem, [pats[i] for i in idx], w)
            bad = [(pats[i], g, want[i]) for i, g in zip(idx, got) if g != want[i]]
            assert not bad, (c.name, w, bad[:5])
    keep, img = mem.put(blob)
    try:
        with engine.FmIndex(ctx, img, len(blob), locate=True) as fm:
            assert fm.info()["flags"] == engine.FM_LOCATE
    except engine.GrlbwtError as e:
        assert e.code == EINVAL, e


# ------------------------------------------------------------------ B, C: small collections the engine builds
class Collection:
    def __init__(self, name, data, w):
        self.name, self.data, self.w = name, np.asarray(data, dtype=DT[w]), w
        self.sep = int(self.data[-1])
        assert self.sep == int(self.data.min())
        self.ends = np.flatnonzero(self.data == self.data[-1])
        self.starts = np.concatenate([[0], self.ends[:-1] + 1])
        self.strings = [self.data[a:b] for a, b in zip(self.starts, self.ends)]        # without their separators
        self.n = len(self.data)

    def matches(self, p):
        """text positions where the pattern starts (a pattern holds the separator as its last cell at most, so a match never
        crosses a string's end)"""
        m = len(p)
        if m == 0 or m > self.n:
            return np.zeros(0, dtype=np.int64)
        win = np.lib.stride_tricks.sliding_window_view(self.data, m)
        return np.flatnonzero((win == np.array(p, dtype=self.data.dtype)).all(axis=1))

    def where(self, x):
        s = np.searchsorted(self.ends, x, side="left")            # separators in front of x = the string's number
        return s, x - self.starts[s]


def make_collections():
    rng = np.random.default_rng(20261018)
    out = {}
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    strs = [acgt[rng.integers(0, 4, size=int(rng.integers(1, 61)))] for _ in range(260)]
    strs += [strs[int(rng.integers(0, 260))] for _ in range(38)] + [acgt[:0], acgt[:0]]
    strs[5] = acgt[rng.integers(0, 4, size=60)]
    order = rng.permutation(len(strs))
    out["dna"] = Collection("dna", np.concatenate([np.concatenate([strs[i], [10]]) for i in order]), 1)
    out["single"] = Collection("single", np.concatenate([acgt[rng.integers(0, 4, size=500)], [10]]), 1)
    one = np.concatenate([acgt[rng.integers(0, 4, size=40)], [10]])
    out["identical"] = Collection("identical", np.tile(one, 64), 1)
    raw = open(os.path.join(HERE, "golden", "test_2bytes_alphabet.txt"), "rb").read()
    out["two_bytes"] = Collection("two_bytes", np.frombuffer(raw, dtype=np.uint16), 2)
    out["wide_u64"] = Collection("wide_u64", wc.collection(rng, 8, 30, 40, 12, 2 ** 30 - 3, 2 ** 63 + 11), 8)
    return out


COLS = make_collections()


def collection_patterns(col):
    """Substrings of the text of 1, 2, 7, 31 cells and whole strings; the same with one cell changed; a whole string and a suffix
    in front of the separator; one pattern longer than any string; the empty one."""
    rng = np.random.default_rng(len(col.data) * 7 + col.w)
    body = sorted(set(int(v) for v in np.unique(col.data)) - {col.sep})
    longest = max(len(s) for s in col.strings)
    pats = []

    def sub(m):
        cand = [s for s in col.strings if len(s) >= m]
        if not cand:
            return None
        s = cand[int(rng.integers(len(cand)))]
        a = int(rng.integers(0, len(s) - m + 1))
        return [int(v) for v in s[a:a + m]]

    def changed(p):
        q = list(p)
        i = int(rng.integers(len(q)))
        other = [v for v in body if v != q[i]] + [max(body) + 1]
        q[i] = other[int(rng.integers(len(other)))]
        return q

    for m in (1, 2, 7, 31):
        for _ in range(8):
            p = sub(min(m, longest))
            pats.append(p)
            if len(pats) % 2 == 0:
                pats.append(changed(p))
    full = [s for s in col.strings if len(s)]
    for _ in range(6):
        s = [int(v) for v in full[int(rng.integers(len(full)))]]
        pats += [s, s + [col.sep], s[len(s) // 2:] + [col.sep]]
        if len(pats) % 2 == 0:
            pats += [changed(s), changed(s) + [col.sep]]
    pats.append([col.sep])
    pats.append([body[i % len(body)] for i in range(longest + 3)])
    pats.append([])
    return pats


_images = {}


def image_of(lib, col, flags):
    key = (lib, col.name, flags)
    if key not in _images:
        with engine.Context(0, flags, lib) as ctx:
            ctx.upload(col.data.tobytes(), col.w)
            ctx.build()
            _images[key] = ctx.result_bytes()
        _, _, sym, ln = bc.parse_rl_bwt(_images[key])
        assert int(ln.sum()) == col.n
    return _images[key]


def expected_counts(col, pats):
    exp = [col.n if not p else len(col.matches(p)) for p in pats]
    hit = sum(1 for e in exp if e)
    assert 2 * hit >= len(pats), (col.name, hit, len(pats))                  # at least half of the patterns occur ...
    assert 10 * (len(pats) - hit) >= len(pats), (col.name, hit, len(pats))   # ... and at least one in ten does not
    return exp


def run_collection(ctx, flags, mem, lib, name):
    """B and C on one collection: counts against the sliding compare, the located (string, offset) sets against its positions"""
    col = COLS[name]
    pats = collection_patterns(col)
    exp = expected_counts(col, pats)
    blob = image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob), locate=True) as fm:
        del keep
        info = fm.info()
        assert (info["n_syms"], info["n_strings"], info["separator"]) == (col.n, len(col.strings), col.sep)
        assert info["sigma"] == len(np.unique(col.data)) and info["idx_bytes"] == (8 if flags & engine.FLAG_FORCE_IDX64 else 4)
        got = count(fm, mem, pats, col.w)
        bad = [(i, pats[i][:8], g, e) for i, (g, e) in enumerate(zip(got, exp)) if g[1] - g[0] != e or (e == 0 and g != (0, 0))]
        assert not bad, (name, bad[:5])
        if col.w < 8:                                              # the same patterns as wider cells
            assert count(fm, mem, pats, 8) == got
        assert got[-1] == (0, col.n) and got[-3] == (0, len(col.strings))
        # C: every row of every range
        rows = np.concatenate([np.arange(a, b, dtype=np.uint64) for a, b in got])
        assert 0 < len(rows) < 200000
        s, o = locate(fm, mem, rows)
        at = 0
        for p, (a, b) in zip(pats, got):
            mine = sorted(zip(s[at:at + b - a].tolist(), o[at:at + b - a].tolist()))
            at += b - a
            if p:
                ws, wo = col.where(col.matches(p))
            else:
                ws, wo = col.where(np.arange(col.n))
            assert mine == sorted(zip(ws.tolist(), wo.tolist())), (name, p[:8])
        if name == "dna":
            dna_rows(fm, mem, col)


def dna_suffix_order(col):
    """(string, offset) of every row: the suffixes with their separator, sorted by content and then by the string's number"""
    keys = []
    for i, s in enumerate(col.strings):
        b = s.tobytes() + b"\n"
        keys += [(b[o:], i, o) for o in range(len(b))]
    keys.sort(key=lambda k: (k[0], k[1]))
    return np.array([k[1] for k in keys], dtype=np.uint64), np.array([k[2] for k in keys], dtype=np.uint64)


_dna_sa = []


def dna_sa(col):
    if not _dna_sa:
        _dna_sa.append(dna_suffix_order(col))
    return _dna_sa[0]


def dna_rows(fm, mem, col):
    """every row against the sorted suffixes; with max_steps = 7 exactly the occurrences at offsets <= 7 resolve"""
    ws, wo = dna_sa(col)
    rows = np.arange(col.n, dtype=np.uint64)
    s, o = locate(fm, mem, rows)
    assert np.array_equal(s, ws) and np.array_equal(o, wo)
    s, o = locate(fm, mem, rows, 7)
    near = wo <= 7
    assert near.any() and (~near).any()
    assert np.array_equal(s[near], ws[near]) and np.array_equal(o[near], wo[near])
    assert bool(np.all(s[~near] == NONE)) and bool(np.all(o[~near] == NONE))
    s, o = locate(fm, mem, rows, 0)
    assert np.array_equal(o[wo == 0], wo[wo == 0]) and bool(np.all(o[wo != 0] == NONE))


# ------------------------------------------------------------------ D: launch shapes
def run_shapes(ctx, flags, mem, lib):
    col = COLS["dna"]
    pats = collection_patterns(col)
    blob = image_of(lib, col, flags)
    keep, img = mem.put(blob)
    ws, wo = dna_sa(col)
    with engine.FmIndex(ctx, img, len(blob), locate=True) as fm:
        base = count(fm, mem, pats, 1)
        for n in SHAPES:
            batch = [pats[i % len(pats)] for i in range(n)]
            assert count(fm, mem, batch, 1) == [base[i % len(pats)] for i in range(n)], n
            rows = (np.arange(n, dtype=np.uint64) * np.uint64(7919)) % np.uint64(col.n)
            s, o = locate(fm, mem, rows)
            assert np.array_equal(s, ws[rows.astype(np.int64)]) and np.array_equal(o, wo[rows.astype(np.int64)]), n


# ------------------------------------------------------------------ E: refusals
def run_refusals(ctx, flags, mem, lib):
    col = COLS["dna"]
    blob = image_of(lib, col, flags)
    keep, img = mem.put(blob)
    A, C_, nl = 65, 67, 10
    with engine.FmIndex(ctx, img, len(blob), locate=True) as fm, engine.FmIndex(ctx, img, len(blob)) as plain:
        # the separator in the middle of pattern 3 (and of pattern 5): nothing is written
        pats = [[A], [A, nl], [], [A, nl, C_], [C_], [nl, nl]]
        cells, off = pack(pats, 1)
        kc, pc = mem.put(cells.tobytes())
        ko, po = mem.put(off.tobytes())
        lo, plo = mem.out(8 * len(pats))
        hi, phi = mem.out(8 * len(pats))
        msg = einval(lambda: fm.count(pc, 1, po, len(pats), plo, phi))
        assert "pattern 3 " in msg, msg
        assert bool(np.all(mem.get(lo) == FILL)) and bool(np.all(mem.get(hi) == FILL))
        # a bad cell width, decreasing offsets
        einval(lambda: fm.count(pc, 3, po, len(pats), plo, phi))
        kd, pd = mem.put(np.array([0, 2, 1, 3], dtype=np.uint64).tobytes())
        einval(lambda: fm.count(pc, 1, pd, 3, plo, phi))
        assert bool(np.all(mem.get(lo) == FILL)) and bool(np.all(mem.get(hi) == FILL))
        # locate without the structures, a row that is not a row
        kr, pr = mem.put(np.array([0, col.n - 1], dtype=np.uint64).tobytes())
        s, ps = mem.out(16)
        o, po2 = mem.out(16)
        einval(lambda: plain.locate(pr, 2, NONE, ps, po2))
        fm.locate(pr, 2, NONE, ps, po2)
        kb, pb = mem.put(np.array([0, col.n], dtype=np.uint64).tobytes())
        s, ps = mem.out(16)
        o, po2 = mem.out(16)
        einval(lambda: fm.locate(pb, 2, NONE, ps, po2))
        assert bool(np.all(mem.get(s) == FILL)) and bool(np.all(mem.get(o) == FILL))
    # an image without a record
    k16, p16 = mem.put(ic.make_image(1, 2, [], []))
    einval(lambda: engine.FmIndex(ctx, p16, 16))
    einval(lambda: engine.FmIndex(ctx, p16, 16, locate=True))
