"""Shared by tests/test_checkpointed_walks_sim.py (serial stand-in) and tests/test_checkpointed_walks_gpu.py (HIP library):
the checkpointed LF walks -- grlbwt_invert_image_checkpointed and the locate index made with GRLBWT_FM_CHECKPOINTS.

The expected values come from the TEXT an image was built from (numpy), never from the engine's other inverter; the checks
that say "agrees with the unsampled call" are the exception and say so.

  1  inversion equals the text, for every collection and sample_bits
  2  the structure the call reports (grlbwt_walk_info), asserted without measured numbers
  3  lane refill under GRLBWT_WALK_LANES (GPU file)
  4  the index: info, counts, every row located, against the text and against the index without checkpoints
  5  foreign images (tests/image_cases.py): same outcome as the calls without checkpoints
  6  refusals

The unsampled index walks a row to the START of its string: on the collections of long strings here that is up to 300 000
dependent steps per row, which is what the feature replaces.  The serial stand-in cannot afford that for every row: there the
byte-for-byte comparison with the unsampled index runs under max_steps = 0 and 64 on those collections (both calls are bounded
by it).  On the GPU, and on the small collections everywhere, it also runs without a bound.
"""
import numpy as np

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic

EINVAL = -22
NONE = fc.NONE
INVERT_BITS = (1, 4, 6, 10, 0)
INDEX_BITS = (2, 6, 0)
EDGE_M = (2, 63, 64, 65, 129)
LANES = ("64", "320", None)
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ the checkpoint rule, by the issue's definition
def mix(j):
    z = (j + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pick(j, n, b):
    """the row picked in block j of 2^b rows (the last block may be shorter: the offset is reduced modulo its length)"""
    s = 1 << b
    ln = min(s, n - j * s)
    return j * s + (mix(j) & (s - 1)) % ln


def ceil_log2(x):
    return (x - 1).bit_length() if x > 1 else 0


# ------------------------------------------------------------------ collections
def make_collections():
    rng = np.random.default_rng(20261019)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    nl = np.array([10], dtype=np.uint8)

    def rand(m):
        return acgt[rng.integers(0, 4, size=m)]

    def coll(name, strs):
        return fc.Collection(name, np.concatenate([np.concatenate([s, nl]) for s in strs]), 1)

    out = {k: fc.COLS[k] for k in ("dna", "identical", "two_bytes", "wide_u64")}
    out["one_long"] = coll("one_long", [rand(200000)])
    out["mixed"] = coll("mixed", [rand(300000), rand(0), rand(70000), rand(1), rand(63)])
    unit = rand(1500)
    rep = np.tile(unit, 200)
    hit = np.flatnonzero(rng.random(len(rep)) < 0.001)
    rep[hit] = acgt[(np.searchsorted(acgt, rep[hit]) + 1 + rng.integers(0, 3, size=len(hit))) % 4]
    assert 100 < len(hit) < 600 and not np.array_equal(rep[:1500], rep[1500:3000])
    out["repeats"] = coll("repeats", [rep, np.concatenate([np.repeat(acgt[:1], 5000), np.tile(acgt, 2000)])])
    for m in EDGE_M:             # one string: n_checkpoints = 1 + ceil(n / 16) = m at sample_bits = 4, the last block partly filled
        n = 16 * (m - 1) - 7
        out["edge_m%d" % m] = coll("edge_m%d" % m, [rand(n - 1)])
        assert 1 + -(-out["edge_m%d" % m].n // 16) == m
    return out


COLS = make_collections()
NAMES = list(COLS)
LARGE = ("one_long", "mixed", "repeats")
REFILL = ["mixed", "repeats"] + ["edge_m%d" % m for m in EDGE_M]
assert max(c.n for c in COLS.values()) < 420000


# ------------------------------------------------------------------ 2: the structure a call reports
def check_info(info, col, bits, on_gpu, lanes=None, index=False):
    n, k = col.n, len(col.strings)
    b = info["sample_bits"]
    assert (b == bits) if bits else (1 <= b <= 20), info
    m = k + -(-n // (1 << b))
    assert (info["n_strings"], info["n_checkpoints"]) == (k, m), info
    assert info["longest_segment"] <= n
    assert info["jump_rounds"] <= ceil_log2(m), info
    assert 1 <= info["longest_chain"] <= m
    if k == 1:                   # one chain holds every checkpoint that is not void (a block's pick below k: the row is a head)
        void = sum(1 for j in range(m - k) if pick(j, n, b) < k)
        assert void <= 1 and info["longest_chain"] == m - void, (info, void)
        assert info["jump_rounds"] >= ceil_log2(info["longest_chain"]) - 1, info
    if on_gpu:
        up = -(-m // 64) * 64
        assert info["walk_lanes"] % 64 == 0 and 64 <= info["walk_lanes"] <= up, info
        if lanes:
            assert info["walk_lanes"] == min(-(-int(lanes) // 64) * 64, up), info
    else:
        assert info["walk_lanes"] == m, info
    assert info["lane_refills"] == max(0, m - info["walk_lanes"]), info
    assert info["scratch_bytes"] > 0
    if index:
        assert info["sample_bytes"] == 2 * m * (8 if index == 8 else 4), info
    else:
        assert info["sample_bytes"] == 0


# ------------------------------------------------------------------ 1: inversion equals the text
def run_invert(ctx, flags, mem, lib, name, bits, lanes=None):
    col = COLS[name]
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    out, pout = mem.out(col.n * col.w)
    n, info = ctx.invert_image_checkpointed(img, len(blob), col.w, pout, col.n, sample_bits=bits)
    assert n == col.n
    got = mem.body(out, col.n * col.w)
    assert got.tobytes() == col.data.tobytes(), (name, bits, int(np.flatnonzero(got != col.data.view(np.uint8))[0]))
    check_info(info, col, bits, mem.on_gpu, lanes)
    return info


# ------------------------------------------------------------------ 4: the index
def suffix_order(col):
    """(string, offset) of every row: the suffixes with their separator, by content and then by the string's number"""
    keys = []
    for i, s in enumerate(col.strings):
        t = tuple(int(v) for v in s) + (col.sep,)
        keys += [(t[o:], i, o) for o in range(len(t))]
    keys.sort(key=lambda q: (q[0], q[1]))
    return np.array([q[1] for q in keys], dtype=np.uint64), np.array([q[2] for q in keys], dtype=np.uint64)


_sa = {}


def expected_rows(col):
    if col.name not in _sa:
        _sa[col.name] = fc.dna_sa(col) if col.name == "dna" else suffix_order(col)
    return _sa[col.name]


KMER = 6
_kmers, _pats = {}, {}


def patterns_of(col):
    if col.name not in _pats:
        _pats[col.name] = fc.collection_patterns(col)
    return _pats[col.name]


def kmer_codes(col):
    """code of the KMER cells that start at every text position (-1 where they would cross a string's end)"""
    if col.name in _kmers:
        return _kmers[col.name]
    lut = np.full(256, -1, dtype=np.int64)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
    d = lut[col.data]
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([d, np.full(KMER - 1, -1)]), KMER)
    code = (win * (4 ** np.arange(KMER - 1, -1, -1))).sum(axis=1)
    code[(win < 0).any(axis=1)] = -1
    _kmers[col.name] = code
    return code


def check_large_rows(fm, mem, col, rows, s, o):
    """located (string, offset) of `rows` on a collection too large to sort here: the text at the located position starts with
    the pattern whose range the row lies in (all 4^KMER patterns: their ranges hold every row whose suffix has KMER cells
    before its string ends), and no two rows share a position -- all of them: a permutation of the text's positions."""
    k = len(col.strings)
    assert int(s.max()) < k
    lens = np.array([len(x) for x in col.strings], dtype=np.uint64)
    assert bool(np.all(o <= lens[s.astype(np.int64)]))
    x = col.starts[s.astype(np.int64)] + o.astype(np.int64)
    assert len(np.unique(x)) == len(x)
    if len(rows) == col.n:
        assert np.array_equal(np.sort(x), np.arange(col.n))
    pats = [[int(b"ACGT"[(i >> (2 * (KMER - 1 - q))) & 3]) for q in range(KMER)] for i in range(4 ** KMER)]
    ranges = fc.count(fm, mem, pats, 1)
    row_code = np.full(col.n, -1, dtype=np.int64)
    for i, (a, b) in enumerate(ranges):
        row_code[a:b] = i
    want = row_code[rows.astype(np.int64)]
    assert (want >= 0).sum() * 10 >= 9 * len(rows)
    code = kmer_codes(col)
    assert np.array_equal(code[x], want), "a located position does not start with the row's pattern"


def index_rows(col):
    k = len(col.strings)
    if col.name == "mixed":
        return np.unique(np.concatenate([np.arange(k), np.arange(0, col.n, 7)])).astype(np.uint64)
    return np.arange(col.n, dtype=np.uint64)


def run_index(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    k = len(col.strings)
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob), locate=True) as plain, \
            engine.FmIndex(ctx, img, len(blob), locate=True, checkpoints=True, sample_bits=bits) as fm:
        del keep
        a, b = plain.info(), fm.info()
        wi = fm.walk_info()
        idx = 8 if flags & engine.FLAG_FORCE_IDX64 else 4
        check_info(wi, col, bits, mem.on_gpu, index=idx)
        assert b["flags"] == engine.FM_LOCATE | engine.FM_CHECKPOINTS | (bits << 8) and a["flags"] == engine.FM_LOCATE
        assert b["index_bytes"] == a["index_bytes"] + wi["sample_bytes"]
        assert {q: v for q, v in a.items() if q not in ("flags", "index_bytes")} == {q: v for q, v in b.items() if q not in ("flags", "index_bytes")}
        assert (b["n_syms"], b["n_strings"], b["idx_bytes"]) == (col.n, k, idx)
        pats = patterns_of(col)
        assert fc.count(fm, mem, pats, col.w) == fc.count(plain, mem, pats, col.w)
        rows = index_rows(col)
        s, o = fc.locate(fm, mem, rows)
        # the rows [0, k): string i's separator, at the offset that is its length
        assert np.array_equal(s[:k], np.arange(k, dtype=np.uint64))
        assert np.array_equal(o[:k], np.array([len(x) for x in col.strings], dtype=np.uint64))
        if name in LARGE:
            check_large_rows(fm, mem, col, rows, s, o)
            caps = (0, 64, NONE) if mem.on_gpu else (0, 64)
        else:
            ws, wo = expected_rows(col)
            assert np.array_equal(s, ws) and np.array_equal(o, wo), name
            caps = (0, 7, NONE)
        for cap in caps:         # agrees with the unsampled index, byte for byte; and the exact-resolution rule against the text
            s1, o1 = fc.locate(fm, mem, rows, cap)
            s0, o0 = fc.locate(plain, mem, rows, cap)
            assert s1.tobytes() == s0.tobytes() and o1.tobytes() == o0.tobytes(), (name, bits, cap)
            near = o <= np.uint64(cap)
            assert np.array_equal(s1[near], s[near]) and np.array_equal(o1[near], o[near])
            assert bool(np.all(s1[~near] == NONE)) and bool(np.all(o1[~near] == NONE))
            if name == "dna" and cap == 7:
                assert near.any() and (~near).any()


# ------------------------------------------------------------------ 5: foreign images
FOREIGN = [c.name for c in ic.CASES if not c.giant]
FOREIGN_BITS = (1, 6)


def cell_width(c):
    return {1: 1, 2: 2, 3: 4, 4: 4}.get(c.sb, 8)


def _outcome(fn):
    try:
        return None, fn()
    except engine.GrlbwtError as e:
        return e.code, None


def run_foreign(ctx, mem, c):
    blob = c.image()
    keep, img = mem.put(blob)
    w = cell_width(c)

    def invert(bits):
        out, pout = mem.out(c.n * w)
        if bits is None:
            n = ctx.invert_image(img, len(blob), w, pout, c.n)
        else:
            n, info = ctx.invert_image_checkpointed(img, len(blob), w, pout, c.n, sample_bits=bits)
            assert info["n_checkpoints"] == info["n_strings"] + -(-n // (1 << bits))
        assert n == c.n
        return mem.body(out, c.n * w).tobytes()

    base = _outcome(lambda: invert(None))
    for bits in FOREIGN_BITS:
        assert _outcome(lambda: invert(bits)) == base, (c.name, bits, base[0])

    def index(bits):
        rows = np.arange(c.n, dtype=np.uint64)
        kw = {} if bits is None else dict(checkpoints=True, sample_bits=bits)
        with engine.FmIndex(ctx, img, len(blob), locate=True, **kw) as fm:
            info = fm.info()
            got = [fc.locate(fm, mem, rows, cap) for cap in (0, 300)] if c.n else []
            return [info[q] for q in ("n_syms", "n_runs", "n_strings", "sigma", "separator")], [(s.tobytes(), o.tobytes()) for s, o in got]

    base = _outcome(lambda: index(None))
    for bits in FOREIGN_BITS:
        assert _outcome(lambda: index(bits)) == base, (c.name, bits, base[0])
    return base[0]


# ------------------------------------------------------------------ 6: refusals
def run_refusals(ctx, flags, mem, lib):
    col = COLS["dna"]
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    out, pout = mem.out(col.n)
    for bits in (-1, 21):
        fc.einval(lambda: ctx.invert_image_checkpointed(img, len(blob), 1, pout, col.n, sample_bits=bits))
    fc.einval(lambda: ctx.invert_image_checkpointed(img, len(blob), 1, pout, col.n - 1, sample_bits=4))
    fc.einval(lambda: ctx.invert_image_checkpointed(img, len(blob), 3, pout, col.n, sample_bits=4))
    assert bool(np.all(mem.get(out) == fc.FILL))
    fc.einval(lambda: engine.FmIndex(ctx, img, len(blob), locate=False, checkpoints=True))
    fc.einval(lambda: engine.FmIndex(ctx, img, len(blob), locate=True, checkpoints=True, sample_bits=21))
    fc.einval(lambda: engine.FmIndex(ctx, img, len(blob), locate=True, checkpoints=False, sample_bits=4))
    with engine.FmIndex(ctx, img, len(blob), locate=True) as plain:
        with __import__("pytest").raises(engine.GrlbwtError) as e:
            plain.walk_info()
        assert e.value.code == EINVAL
    with engine.FmIndex(ctx, img, len(blob), locate=True, checkpoints=True, sample_bits=20) as fm:      # one block: heads and one pick
        assert fm.walk_info()["n_checkpoints"] == len(col.strings) + 1
