"""Shared by tests/test_fm_sa_sim.py (serial stand-in) and tests/test_fm_sa_gpu.py (HIP library): the document array and the
generalized suffix array of a collection from its FM index (grlbwt_fm_sa).

The collections are those of tests/walk_cases.py, imported.  The expected values come from the TEXT, never from the engine:
walk_cases.expected_rows (a Python sort of the suffixes) on the small collections, a numpy prefix-doubling suffix sort on the
LARGE ones, terminators ordered by the string's number; the two are pinned against each other on every small collection.  The
checks that say "equal to locate" are the exception and say so.  Every row of every window is compared; every output buffer
has guard bytes on both sides.

  1  the whole array against the text: form 0 (LOCATE) and form 1 (LOCATE | CHECKPOINTS), widths (8, 8) and the narrowest
  2  byte for byte what grlbwt_fm_locate gives for rows 0 .. n - 1 on the same index
  3  windows
  4  one output at a time, and the step counts the header states
  5  width refusals, before any store
  6  other refusals
  7  the index is unchanged
  8  lanes (the launch the call reports)
  9  foreign images (tests/image_cases.py)
"""
import ctypes as C

import numpy as np

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import walk_cases as wk

EINVAL = -22
FILL = fc.FILL
DT = fc.DT
FRONT = 64                       # guard bytes in front of an output (a multiple of every width: the output stays aligned)
FORMS = (None,) + tuple(wk.INDEX_BITS)           # None: form 0, an index without checkpoints; else form 1 at these sample_bits
FORM_IDS = ["strings"] + ["segments_b%d" % b for b in wk.INDEX_BITS]
# the windows: both forms on the reads; on the long strings form 1 only (form 0 is one dependent chain of 300 000 steps per call there,
# and twice that with its length pass: the whole-array cases pay it once per width, fourteen windows would pay it fourteen times)
WINDOW_CASES = [("dna", b) for b in FORMS] + [("mixed", b) for b in FORMS if b is not None]
WINDOW_IDS = ["%s-%s" % (n, "strings" if b is None else "segments_b%d" % b) for n, b in WINDOW_CASES]


def make_singles():
    """257 strings of one cell each: string number 256 does not fit one byte"""
    rng = np.random.default_rng(20261020)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    data = np.full(2 * 257, 10, dtype=np.uint8)
    data[0::2] = acgt[rng.integers(0, 4, size=257)]
    return fc.Collection("singles257", data, 1)


SINGLES = make_singles()
COLS = dict(wk.COLS)
COLS[SINGLES.name] = SINGLES
SMALL = [n for n in COLS if n not in wk.LARGE]


# ------------------------------------------------------------------ expected values, from the text
def suffix_sort(col):
    """(string, offset) of every row by prefix doubling over the whole text: a terminator ranks below every cell and among the
    terminators by its string's number, so it equals nothing and no comparison reaches past one"""
    n, k = col.n, len(col.strings)
    _, inv = np.unique(col.data, return_inverse=True)                  # the separator is the smallest value: 0
    rank = inv.astype(np.int64).reshape(-1) + (k - 1)
    rank[col.ends] = np.arange(k)
    h = 1
    while True:
        nxt = np.full(n, -1, dtype=np.int64)
        if h < n:
            nxt[:n - h] = rank[h:]
        order = np.lexsort((nxt, rank))
        a, b = rank[order], nxt[order]
        new = np.concatenate([[0], np.cumsum((a[1:] != a[:-1]) | (b[1:] != b[:-1]))])
        rank = np.empty(n, dtype=np.int64)
        rank[order] = new
        if int(new[-1]) == n - 1:
            break
        h *= 2
    s, o = col.where(order)
    return s.astype(np.uint64), o.astype(np.uint64)


_exp = {}


def expected(col):
    if col.name not in _exp:
        _exp[col.name] = suffix_sort(col) if col.name in wk.LARGE else wk.expected_rows(col)
    return _exp[col.name]


def run_sort_is_pinned(name):
    col = COLS[name]
    ws, wo = wk.expected_rows(col)
    s, o = suffix_sort(col)
    assert np.array_equal(s, ws) and np.array_equal(o, wo), name


def lengths(col):
    return np.array([len(x) for x in col.strings], dtype=np.int64)    # without the separators


def narrowest(v):
    return next(w for w in (1, 2, 4, 8) if w == 8 or v < 1 << (8 * w))


def narrow_widths(col):
    return narrowest(len(col.strings) - 1), narrowest(int(lengths(col).max()))


# ------------------------------------------------------------------ one call, guarded outputs, info checked
def out(mem, nbytes):
    buf, ptr = mem.out(FRONT + nbytes)
    return buf, ptr + FRONT


def body(mem, buf, nbytes):
    h = mem.get(buf)
    assert bool(np.all(h[:FRONT] == FILL)), "bytes in front of the output were written"
    assert bool(np.all(h[FRONT + nbytes:] == FILL)), "bytes behind the output were written"
    return h[FRONT:FRONT + nbytes].copy()


def untouched(mem, buf):
    return bool(np.all(mem.get(buf) == FILL))


def index(ctx, flags, mem, lib, col, bits, **kw):
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    if bits is not None:
        kw.update(checkpoints=True, sample_bits=bits)
    return engine.FmIndex(ctx, img, len(blob), locate=True, **kw)


def call(fm, mem, n, rb=0, re=None, ws=8, wo=8, da=True, sa=True):
    """grlbwt_fm_sa on rows [rb, re) -> (strings, offsets, info); an output that is not asked for comes back as None, its buffer
    (still handed a width) checked for the fill"""
    cnt = (n if re is None or re == engine.UINT64_MAX else re) - rb
    sb, sp = out(mem, cnt * ws)
    ob, op = out(mem, cnt * wo)
    fm.suffix_array(rb, re, ws, sp if da else None, wo, op if sa else None)
    s = body(mem, sb, cnt * ws).view(DT[ws])
    o = body(mem, ob, cnt * wo).view(DT[wo])
    if not da:
        assert untouched(mem, sb)
    if not sa:
        assert untouched(mem, ob)
    return (s if da else None), (o if sa else None), fm.sa_info()


def tickets_of(col, fm, bits):
    return len(col.strings) if bits is None else fm.walk_info()["n_checkpoints"]


def check_lanes(info, tickets, on_gpu, lanes=None):
    """the launch, by the rule of walk_cases.check_info"""
    if on_gpu:
        up = -(-tickets // 64) * 64
        assert info["walk_lanes"] % 64 == 0 and 64 <= info["walk_lanes"] <= up, info
        if lanes:
            assert info["walk_lanes"] == min(-(-int(lanes) // 64) * 64, up), info
    else:
        assert info["walk_lanes"] == tickets, info
    assert info["lane_refills"] == max(0, tickets - info["walk_lanes"]), info


def check(col, fm, bits, got, rb, re, ws, wo, on_gpu, lanes=None, extract=False):
    """the outputs of one call against the text, and everything its info states"""
    s, o, info = got
    n, k = col.n, len(col.strings)
    end = n if re is None or re == engine.UINT64_MAX else re
    es, eo = expected(col)
    for g, e, w in ((s, es, ws), (o, eo, wo)):
        if g is None:
            continue
        want = e[rb:end]
        assert int(want.max(initial=0)) < 1 << (8 * w) or w == 8
        bad = np.flatnonzero(g.astype(np.uint64) != want)
        assert not len(bad), (col.name, bits, len(bad), bad[:5], g[bad[:5]], want[bad[:5]])
        fill = int.from_bytes(bytes([FILL]) * w, "little")
        assert not bool(np.any((g.astype(np.uint64) == np.uint64(fill)) & (want != np.uint64(fill)))), "an entry keeps the fill"
    assert (info["n_rows"], info["n_strings"], info["row_begin"], info["row_end"], info["n_written"]) == (n, k, rb, end, end - rb), info
    assert (info["string_bytes"], info["offset_bytes"]) == (ws if s is not None else 0, wo if o is not None else 0), info
    assert info["form"] == (0 if bits is None else 1), info
    if end == rb:                # an empty window runs no walk
        assert (info["walk_steps"], info["longest_walk"], info["walk_lanes"], info["lane_refills"]) == (0, 0, 0, 0), info
        return
    # a walk stops AT the separator's row: a string of L cells takes L - 1 steps.  Form 1 takes n - k (the header's count), form 0
    # the same, and twice that where a length pass comes first: offsets on an index that keeps no lengths.
    twice = bits is None and o is not None and not extract
    assert info["walk_steps"] == (2 if twice else 1) * (n - k), info
    if bits is None:
        assert info["longest_walk"] == int(lengths(col).max()), info
    else:
        assert info["longest_walk"] == fm.walk_info()["longest_segment"], info
        assert n - fm.walk_info()["n_checkpoints"] <= info["walk_steps"] <= n
    check_lanes(info, tickets_of(col, fm, bits), on_gpu, lanes)
    assert info["scratch_bytes"] > 0


# ------------------------------------------------------------------ 1: the whole array against the text
def run_whole(ctx, flags, mem, lib, name, bits, lanes=None):
    col = COLS[name]
    with index(ctx, flags, mem, lib, col, bits) as fm:
        for ws, wo in ((8, 8), narrow_widths(col)):
            check(col, fm, bits, call(fm, mem, col.n, 0, None, ws, wo), 0, None, ws, wo, mem.on_gpu, lanes)


# ------------------------------------------------------------------ 2: equal to locate
def run_equals_locate(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    with index(ctx, flags, mem, lib, col, bits) as fm:
        ls, lo = fc.locate(fm, mem, np.arange(col.n, dtype=np.uint64))
        s, o, _ = call(fm, mem, col.n)
        assert s.tobytes() == ls.tobytes() and o.tobytes() == lo.tobytes(), (name, bits)


# ------------------------------------------------------------------ 3: windows
def windows(n, k):
    return [(0, 0), (n, n), (0, n), (k - 1, k + 1), (1, n - 1), (63, 65), (64, 128), (n - 1, n)]


def run_windows(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    n = col.n
    assert n > 128
    ws, wo = narrow_widths(col)
    with index(ctx, flags, mem, lib, col, bits) as fm:
        for rb, re in windows(n, len(col.strings)):
            check(col, fm, bits, call(fm, mem, n, rb, re, ws, wo), rb, re, ws, wo, mem.on_gpu)
        for rb in (0, n - 1, n):                                  # row_end = UINT64_MAX means n, given or by default
            check(col, fm, bits, call(fm, mem, n, rb, engine.UINT64_MAX, 8, 8), rb, None, 8, 8, mem.on_gpu)
            check(col, fm, bits, call(fm, mem, n, rb, None, 8, 8), rb, None, 8, 8, mem.on_gpu)


# ------------------------------------------------------------------ 4: one output at a time
def run_one_output(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    n, k = col.n, len(col.strings)
    ws, wo = narrow_widths(col)
    with index(ctx, flags, mem, lib, col, bits) as fm:
        da = call(fm, mem, n, 0, None, ws, wo, sa=False)
        check(col, fm, bits, da, 0, None, ws, wo, mem.on_gpu)
        assert da[1] is None and da[2]["offset_bytes"] == 0 and da[2]["walk_steps"] == n - k       # no length pass
        sa = call(fm, mem, n, 0, None, ws, wo, da=False)
        check(col, fm, bits, sa, 0, None, ws, wo, mem.on_gpu)
        assert sa[0] is None and sa[2]["string_bytes"] == 0
        assert sa[2]["walk_steps"] == (2 * (n - k) if bits is None else n - k)
        # the absent output's width is ignored, whatever it is
        ob, op = out(mem, n * wo)
        fm.suffix_array(0, None, 3, None, wo, op)
        assert body(mem, ob, n * wo).tobytes() == sa[1].tobytes() and fm.sa_info() == sa[2]
    if bits is None:             # an index that extracts keeps the strings' starts: the lengths without a pass
        with index(ctx, flags, mem, lib, col, None, extract=True) as fm:
            got = call(fm, mem, n, 0, None, ws, wo)
            check(col, fm, None, got, 0, None, ws, wo, mem.on_gpu, extract=True)
            assert got[2]["walk_steps"] == n - k


# ------------------------------------------------------------------ 5: width refusals, before any store
def run_width_refusals(ctx, flags, mem, lib, bits):
    for name, ws, wo, word in (("mixed", 8, 1, "offset_bytes = 1"), ("one_long", 8, 2, "offset_bytes = 2"), (SINGLES.name, 1, 8, "string_bytes = 1")):
        col = COLS[name]
        n = col.n
        with index(ctx, flags, mem, lib, col, bits) as fm:
            sb, sp = out(mem, n * ws)
            ob, op = out(mem, n * wo)
            msg = fc.einval(lambda: fm.suffix_array(0, None, ws, sp, wo, op))
            assert word in msg, msg
            big = {"mixed": 300000, "one_long": 200000, SINGLES.name: 256}[name]
            assert str(big) in msg, msg                            # the message names the value that does not fit
            assert untouched(mem, sb) and untouched(mem, ob)
            if name == SINGLES.name:                               # ... and as the only output
                fc.einval(lambda: fm.suffix_array(0, None, 1, sp, 8, None))
                assert untouched(mem, sb)
                check(col, fm, bits, call(fm, mem, n, 0, None, 2, 1), 0, None, 2, 1, mem.on_gpu)
            else:
                fc.einval(lambda: fm.suffix_array(0, None, 8, None, wo, op))
                assert untouched(mem, ob)
                check(col, fm, bits, call(fm, mem, n, 0, None, 1, 4), 0, None, 1, 4, mem.on_gpu)


# ------------------------------------------------------------------ 6: other refusals
def run_refusals(ctx, flags, mem, lib, bits):
    col = COLS["dna"]
    n = col.n
    L = ctx.L
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    sb, sp = out(mem, 8 * n)
    ob, op = out(mem, 8 * n)

    def clean():
        return untouched(mem, sb) and untouched(mem, ob)

    with engine.FmIndex(ctx, img, len(blob)) as plain:             # an index without the locate structures
        msg = fc.einval(lambda: plain.suffix_array(0, None, 8, sp, 8, op))
        assert "locating" in msg, msg
    with index(ctx, flags, mem, lib, col, bits) as fm:
        fc.einval(lambda: fm.suffix_array(0, None, 8, None, 8, None))               # no output
        for w in (0, 3, 16):
            msg = fc.einval(lambda: fm.suffix_array(0, None, w, sp, 8, op))
            assert "string_bytes is %d" % w in msg, msg
            msg = fc.einval(lambda: fm.suffix_array(0, None, 8, sp, w, op))
            assert "offset_bytes is %d" % w in msg, msg
            fc.einval(lambda: fm.suffix_array(0, None, w, sp, 8, None))
            fc.einval(lambda: fm.suffix_array(0, None, 8, None, w, op))
        msg = fc.einval(lambda: fm.suffix_array(5, 4, 8, sp, 8, op))
        assert "[5, 4)" in msg, msg
        msg = fc.einval(lambda: fm.suffix_array(0, n + 1, 8, sp, 8, op))
        assert "%d)" % (n + 1) in msg, msg
        fc.einval(lambda: fm.suffix_array(n + 1, n + 1, 8, sp, 8, op))
        fc.einval(lambda: fm.suffix_array(0, None, 8, sp + 4, 8, op))               # an output that is not aligned to its width
        assert clean()
        assert L.grlbwt_fm_sa(ctx._h, None, 0, n, 8, C.c_void_p(sp), 8, C.c_void_p(op)) == EINVAL      # a null index
        assert L.grlbwt_fm_sa_info_get(None, None) == EINVAL
        assert clean()
        check(col, fm, bits, call(fm, mem, n), 0, None, 8, 8, mem.on_gpu)                # the index still answers


# ------------------------------------------------------------------ 7: the index is unchanged
def run_index_unchanged(ctx, flags, mem, lib):
    """after lcp_cases.run_index_unchanged: info (index_bytes), a count batch and a locate batch, before and after"""
    col = COLS["dna"]
    n = col.n
    pats = fc.collection_patterns(col)
    rows = (np.arange(500, dtype=np.uint64) * np.uint64(7919)) % np.uint64(n)
    blob = fc.image_of(lib, col, flags)
    for kw in ({"locate": True}, {"locate": True, "checkpoints": True, "sample_bits": 3}, {"locate": True, "extract": True},
               {"locate": True, "checkpoints": True, "sample_bits": 3, "extract": True}):
        keep, img = mem.put(blob)
        bits = kw.get("sample_bits")
        with engine.FmIndex(ctx, img, len(blob), **kw) as fm:
            del keep
            before, counts = fm.info(), fc.count(fm, mem, pats, 1)
            s0, o0 = fc.locate(fm, mem, rows)
            check(col, fm, bits, call(fm, mem, n), 0, None, 8, 8, mem.on_gpu, extract="extract" in kw)
            check(col, fm, bits, call(fm, mem, n, 7, n - 3, 2, 1), 7, n - 3, 2, 1, mem.on_gpu, extract="extract" in kw)
            assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts, kw
            s1, o1 = fc.locate(fm, mem, rows)
            assert s1.tobytes() == s0.tobytes() and o1.tobytes() == o0.tobytes(), kw
            fc.dna_rows(fm, mem, col)


# ------------------------------------------------------------------ 9: foreign images
FOREIGN_BITS = (None,) + wk.FOREIGN_BITS


def run_foreign(ctx, mem, c):
    """Where fm_create(..., LOCATE) succeeds the arrays equal locate over all rows (the rows on no string's chain included: they
    have no position in either call); where it refuses there is nothing to call.  Returns the indexes compared and the rows
    without a position they held."""
    blob = c.image()
    done = lost = 0
    for bits in FOREIGN_BITS:
        keep, img = mem.put(blob)
        kw = {} if bits is None else dict(checkpoints=True, sample_bits=bits)
        try:
            fm = engine.FmIndex(ctx, img, len(blob), locate=True, **kw)
        except engine.GrlbwtError as e:
            assert e.code == EINVAL, e
            continue
        with fm:
            n = fm.info()["n_syms"]
            assert n == c.n
            s, o, info = call(fm, mem, n)
            assert info["n_written"] == n
            if n:
                ls, lo = fc.locate(fm, mem, np.arange(n, dtype=np.uint64))
                assert s.tobytes() == ls.tobytes() and o.tobytes() == lo.tobytes(), (c.name, bits)
                lost += int((ls == np.uint64(fc.NONE)).sum())
                s2, _, _ = call(fm, mem, n, sa=False)
                assert s2.tobytes() == ls.tobytes(), (c.name, bits)
                mid = n // 2
                s3, o3, _ = call(fm, mem, n, mid, n)
                assert s3.tobytes() == ls[mid:].tobytes() and o3.tobytes() == lo[mid:].tobytes(), (c.name, bits)
            done += 1
    return done, lost
