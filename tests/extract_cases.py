"""Shared by tests/test_fm_extract_sim.py (serial stand-in) and tests/test_fm_extract_gpu.py (HIP library): grlbwt_fm_extract,
grlbwt_fm_string_lengths and grlbwt_fm_extract_info_get on an index made with GRLBWT_FM_EXTRACT.

The expected cells come from the TEXT an image was built from (col.data through col.starts), never from another engine call.
The one use of other engine calls is sample_positions(): the absolute positions Q of the index's samples, found by locating the
rows [0, k) and the non-void picks of the checkpoint rule; Q chooses inputs and gives the expected n_pieces, never a cell.
(The foreign images have no text: there the inverter's output stands in, and the test says so.)

  1  every string whole: the output is the text, the offsets are the strings' starts
  2  edges around every sample and around the strings' ends, empty ranges, clamped ends
  3  piece accounting: n_pieces, n_cells, walk_steps, n_samples against numpy -- checked on EVERY call below, by check()
  4  launch shapes and, on the GPU, lane refill
  5  round trip: located occurrences extract to their pattern
  6  cell widths and output alignment
  7  refusals, with nothing written, and the memory accounting
  8  foreign images

A range without a walked cell (empty, or the separator alone) has no piece; every other range has #{q in Q: B < q < E'} + 1.
"""
import numpy as np

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import walk_cases as wk

EINVAL = -22
MAX = fc.NONE
DT = fc.DT
INDEX_BITS = wk.INDEX_BITS
SMALL = [n for n in wk.NAMES if n not in wk.LARGE]
EDGE = ["edge_m%d" % m for m in wk.EDGE_M]
SHAPES = fc.SHAPES
FORMS = [(n, b) for n in wk.NAMES for b in INDEX_BITS] + [(n, None) for n in SMALL]      # bits None: no checkpoints


def form_id(f):
    return "%s-%s" % (f[0], "heads" if f[1] is None else "b%d" % f[1])


def make_index(ctx, flags, mem, lib, col, bits, extract=True):
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    kw = {} if bits is None else dict(checkpoints=True, sample_bits=bits)
    return engine.FmIndex(ctx, img, len(blob), locate=True, extract=extract, **kw)


def slens(col):
    return np.array([len(s) + 1 for s in col.strings], dtype=np.int64)


# ------------------------------------------------------------------ the samples, through existing calls
def sample_positions(fm, mem, col, bits):
    k = len(col.strings)
    rows = list(range(k))
    if bits is not None:
        b = fm.walk_info()["sample_bits"]
        assert (b == bits) if bits else (1 <= b <= 20)
        picks = [wk.pick(j, col.n, b) for j in range(-(-col.n // (1 << b)))]
        rows += [r for r in picks if r >= k]
    s, o = fc.locate(fm, mem, np.array(rows, dtype=np.uint64))
    assert int(s.max()) < k
    q = np.sort(col.starts[s.astype(np.int64)] + o.astype(np.int64))
    assert len(np.unique(q)) == len(q)
    heads = col.starts + slens(col) - 1
    assert np.isin(heads, q).all()                       # every string's separator is a sample
    return q


# ------------------------------------------------------------------ one call, checked against the text
def plan(col, Q, ranges):
    """numpy: per range the expected text slice bounds and its pieces, skip and steps"""
    r = np.asarray(ranges, dtype=np.uint64).reshape(-1, 3)
    s = r[:, 0].astype(np.int64)
    ln = slens(col)[s]
    e = np.minimum(r[:, 2], ln.astype(np.uint64)).astype(np.int64)
    b = np.minimum(r[:, 1], e.astype(np.uint64)).astype(np.int64)
    B, E = col.starts[s] + b, col.starts[s] + e
    sep = (b < e) & (E == col.starts[s] + ln)
    Ew = E - sep
    walked = B < Ew
    top = np.searchsorted(Q, Ew, side="left")
    pieces = np.where(walked, top - np.searchsorted(Q, B, side="right") + 1, 0)
    qtop = Q[np.minimum(top, len(Q) - 1)]
    skip = np.where(walked, qtop - Ew, 0)
    steps = np.where(walked, qtop - B, 0)
    return B, E, pieces, skip, steps


def upload_ranges(mem, ranges):
    r = np.asarray(ranges, dtype=np.uint64).reshape(-1, 3)
    keep = [mem.put(np.ascontiguousarray(r[:, j]).tobytes()) for j in range(3)]
    return r, keep


def run_extract(fm, mem, ranges, w, capacity, shift=0):
    """the call alone: (cells, offsets, n_cells); the bytes in front of and behind both outputs are checked"""
    r, keep = upload_ranges(mem, ranges)
    n, at = len(r), shift * w
    out, pout = mem.out(at + capacity * w)
    off, poff = mem.out(8 * (n + 1))
    got = fm.extract(keep[0][1], keep[1][1], keep[2][1], n, w, pout + at, capacity, poff)
    body = mem.body(out, at + capacity * w)
    assert bool((body[:at] == fc.FILL).all()), "bytes in front of the output were written"
    offs = mem.body(off, 8 * (n + 1)).view(np.uint64)
    assert bool((body[at + got * w:] == fc.FILL).all()), "cells behind the last range were written"
    return body[at:at + got * w].view(DT[w]), offs, got


def check(fm, mem, col, Q, ranges, w=None, shift=0, on_gpu=False):
    """extract `ranges` and compare everything the call and its info report with the text and with numpy's plan"""
    w = w or col.w
    r = np.asarray(ranges, dtype=np.uint64).reshape(-1, 3)
    B, E, pieces, skip, steps = plan(col, Q, r)
    want_off = np.concatenate([[0], np.cumsum(E - B)]).astype(np.uint64)
    total = int(want_off[-1])
    cells, offs, got = run_extract(fm, mem, r, w, total, shift)
    assert got == total and np.array_equal(offs, want_off)
    if len(r) and int((E - B).max()) * 8 >= total:       # few long ranges: slices; many short ones: one gather
        want = np.concatenate([col.data[a:z] for a, z in zip(B, E)]) if total else col.data[:0]
    else:
        lens = E - B
        want = col.data[np.repeat(B - want_off[:-1].astype(np.int64), lens) + np.arange(total)] if total else col.data[:0]
    bad = np.flatnonzero(cells != want.astype(DT[w]))
    assert not len(bad), (col.name, len(bad), int(bad[0]), int(np.searchsorted(want_off, bad[0], side="right") - 1))
    xi = fm.extract_info()
    assert (xi["n_ranges"], xi["n_cells"], xi["n_samples"]) == (len(r), total, len(Q)), xi
    assert xi["n_pieces"] == int(pieces.sum()) and xi["walk_steps"] == int(steps.sum()), (xi, int(pieces.sum()), int(steps.sum()))
    if on_gpu:
        up = -(-xi["n_pieces"] // 64) * 64
        assert xi["walk_lanes"] % 64 == 0 and xi["walk_lanes"] <= up and (xi["walk_lanes"] >= 64 or not xi["n_pieces"]), xi
    else:
        assert xi["walk_lanes"] == xi["n_pieces"], xi
    assert xi["lane_refills"] == max(0, xi["n_pieces"] - xi["walk_lanes"]), xi
    return xi, (pieces, skip)


# ------------------------------------------------------------------ 1: every string whole
def run_whole(ctx, flags, mem, lib, name, bits):
    col = wk.COLS[name]
    k = len(col.strings)
    with make_index(ctx, flags, mem, lib, col, bits) as fm:
        Q = sample_positions(fm, mem, col, bits)
        ranges = [(s, 0, MAX) for s in range(k)]
        xi, _ = check(fm, mem, col, Q, ranges, on_gpu=mem.on_gpu)
        cells, offs, got = run_extract(fm, mem, ranges, col.w, col.n)      # the output IS the text, the offsets are T
        assert cells.tobytes() == col.data.tobytes()
        assert np.array_equal(offs, np.concatenate([col.starts, [col.n]]).astype(np.uint64))
        ln, pl = mem.out(8 * k)
        fm.string_lengths(pl)
        assert np.array_equal(mem.body(ln, 8 * k).view(np.uint64), slens(col).astype(np.uint64))
        return xi


# ------------------------------------------------------------------ 2: edges
def edge_ranges(col, Q, every=False):
    rng = np.random.default_rng(len(Q) * 31 + col.n)
    qs = Q if every or len(Q) <= 200 else Q[np.sort(rng.choice(len(Q), size=200, replace=False))]
    s = np.searchsorted(col.ends, qs, side="left")
    oq = qs - col.starts[s]
    out = []
    for si, o in zip(s.tolist(), oq.tolist()):
        out += [(si, b, e) for b in (o - 1, o, o + 1) for e in (o - 1, o, o + 1) if b >= 0 and e >= 0]
    ln = slens(col)
    pick = np.arange(len(ln)) if len(ln) <= 40 else np.unique(np.concatenate([rng.choice(len(ln), size=40, replace=False), np.flatnonzero(ln == 1)]))
    for si in pick.tolist():
        n = int(ln[si])
        out += [(si, n - 1, n), (si, max(n - 2, 0), n), (si, 0, 1), (si, 0, MAX), (si, n - 1, MAX), (si, n, MAX), (si, n + 5, MAX),
                (si, MAX, MAX), (si, 0, n + 7), (si, n // 2, n // 2), (si, n // 2 + 1, n // 2), (si, n, n - 1), (si, 0, 0)]
    return out


def run_edges(ctx, flags, mem, lib, name, bits):
    col = wk.COLS[name]
    with make_index(ctx, flags, mem, lib, col, bits) as fm:
        Q = sample_positions(fm, mem, col, bits)
        ranges = edge_ranges(col, Q, every=name in EDGE)
        assert len(ranges) >= min(len(Q), 200) * 4
        check(fm, mem, col, Q, ranges, on_gpu=mem.on_gpu)


MIXED_HEADS = [(0, 299990, MAX), (0, 299999, 300000), (0, 300000, 300001), (0, 150000, 150003), (0, 0, 1), (1, 0, MAX), (1, 0, 0), (1, 1, 2),
               (2, 0, MAX), (2, 69990, 70001), (3, 0, MAX), (3, 1, 2), (4, 0, MAX), (4, 62, 64), (4, 64, 70), (2, 35000, 35010)]


# ------------------------------------------------------------------ 3: piece accounting, on the recipe
def run_accounting(ctx, flags, mem, lib):
    col = wk.COLS["mixed"]
    with make_index(ctx, flags, mem, lib, col, 2) as fm:
        Q = sample_positions(fm, mem, col, 2)
        inside = Q[(Q > 1000) & (Q < 299000)]
        gap = int(np.flatnonzero(np.diff(inside) >= 3)[0])      # two neighbouring samples with cells between them
        a, z = int(inside[gap]), int(inside[gap + 1])
        ranges = [(0, 0, MAX), (0, a + 1, z - 1), (0, a, z), (0, a - 1, z + 1), (0, 5, 5), (1, 0, MAX), (3, 0, 1), (2, 10, 60000)]
        xi, (pieces, skip) = check(fm, mem, col, Q, ranges, on_gpu=mem.on_gpu)
        assert pieces[0] >= 1000 and pieces[1] == 1 and skip[1] == 1 and pieces[2] == 1 and skip[2] == 0 and pieces[3] == 3
        assert pieces[4] == 0 and pieces[5] == 0 and (skip > 0).any()
        assert xi["n_pieces"] == int(pieces.sum()) >= 1000


# ------------------------------------------------------------------ 4: launch shapes
def shape_ranges(col, n, seed):
    rng = np.random.default_rng(seed)
    ln = slens(col)
    s = rng.integers(0, len(ln), size=n)
    if n:
        s[rng.random(n) < 0.5] = int(np.argmax(ln))      # half of them in the longest string
    kind = rng.integers(0, 10, size=n)
    length = np.where(kind < 6, rng.integers(0, 40, size=n), np.where(kind < 9, rng.integers(40, 400, size=n), rng.integers(400, 6000, size=n)))
    b = (rng.random(n) * (ln[s] + 2)).astype(np.int64)
    return np.stack([s, b, b + length], axis=1).astype(np.uint64)


def run_shapes(ctx, flags, mem, lib, name, bits, lanes=None):
    col = wk.COLS[name]
    out = []
    with make_index(ctx, flags, mem, lib, col, bits) as fm:
        Q = sample_positions(fm, mem, col, bits)
        for n in SHAPES:
            xi, _ = check(fm, mem, col, Q, shape_ranges(col, n, 1000 + n), on_gpu=mem.on_gpu)
            if n == 0:
                assert (xi["n_pieces"], xi["n_cells"], xi["walk_lanes"]) == (0, 0, 0)
            if lanes:
                assert xi["walk_lanes"] == min(-(-int(lanes) // 64) * 64, -(-xi["n_pieces"] // 64) * 64), (n, xi)
            out.append(xi)
        xi, _ = check(fm, mem, col, Q, [(int(np.argmax(slens(col))), 0, MAX)], on_gpu=mem.on_gpu)      # the long range
        if lanes:
            assert xi["walk_lanes"] == min(-(-int(lanes) // 64) * 64, -(-xi["n_pieces"] // 64) * 64), xi
        out.append(xi)
    return out


# ------------------------------------------------------------------ 5: round trip with locate
def run_round_trip(ctx, flags, mem, lib, name, bits, cap=None):
    """cap: at most that many rows of a pattern's range, evenly spread (the serial stand-in takes microseconds per walk: the one-cell
    patterns of `mixed` have 90 000 rows each); None: every row"""
    col = wk.COLS[name]
    pats = wk.patterns_of(col)
    with make_index(ctx, flags, mem, lib, col, bits) as fm:
        Q = sample_positions(fm, mem, col, bits)
        got = fc.count(fm, mem, pats, col.w)
        hit = [(p, a, b) for p, (a, b) in zip(pats, got) if b > a]
        assert len(hit) >= 20
        per = [np.arange(a, b, dtype=np.uint64) if not cap or b - a <= cap else np.unique(np.linspace(a, b - 1, cap).astype(np.uint64)) for _, a, b in hit]
        rows = np.concatenate(per)
        s, o = fc.locate(fm, mem, rows)
        parts, at = [], 0
        for (p, a, b), mine in zip(hit, per):
            m = len(mine)
            ss, oo = s[at:at + m], o[at:at + m]
            at += m
            parts.append((p, len(p), np.stack([ss, oo, oo + np.uint64(len(p))], axis=1)))
            if p and p[-1] == col.sep:
                parts.append((p[:-1], len(p) - 1, np.stack([ss, oo, oo + np.uint64(len(p) - 1)], axis=1)))
        assert any(len(p) > 1 and p[-1] == col.sep for p, _, _ in hit) and any(not p for p, _, _ in hit)
        ranges = np.concatenate([r for _, _, r in parts])
        check(fm, mem, col, Q, ranges, on_gpu=mem.on_gpu)      # against the text ...
        cells, offs, n = run_extract(fm, mem, ranges, col.w, int(sum(m * len(r) for _, m, r in parts)))
        at = 0
        for p, m, r in parts:                                  # ... and against the pattern, for every occurrence
            blk = cells[at:at + m * len(r)].reshape(len(r), m)
            at += m * len(r)
            assert bool((blk == np.array(p, dtype=cells.dtype)[None, :]).all()), (name, p[:8])
        assert at == n


# ------------------------------------------------------------------ 6: cell widths, alignment
def run_widths(ctx, flags, mem, lib):
    col = wk.COLS["dna"]
    with make_index(ctx, flags, mem, lib, col, 3) as fm:
        Q = sample_positions(fm, mem, col, 3)
        ranges = np.concatenate([shape_ranges(col, 300, 77), np.array([(s, 0, MAX) for s in range(len(col.strings))], dtype=np.uint64)])
        for w in (1, 2, 4, 8):
            for shift in ((0, 1, 2, 3, 4, 7) if w <= 2 else (0, 1)):
                check(fm, mem, col, Q, ranges, w=w, shift=shift, on_gpu=mem.on_gpu)
    for name, w_ok, w_bad in (("two_bytes", 2, 1), ("wide_u64", 8, 4)):
        col = wk.COLS[name]
        with make_index(ctx, flags, mem, lib, col, 3) as fm:
            Q = sample_positions(fm, mem, col, 3)
            ranges = [(s, 0, MAX) for s in range(len(col.strings))]
            for shift in (0, 1, 2, 3, 4, 7):
                check(fm, mem, col, Q, ranges, w=w_ok, shift=shift, on_gpu=mem.on_gpu)
            if name == "two_bytes":
                check(fm, mem, col, Q, ranges, w=8, on_gpu=mem.on_gpu)
            msg = refused(fm, mem, ranges, w_bad, col.n)
            assert "largest symbol does not fit the cell width" in msg, msg


# ------------------------------------------------------------------ 7: refusals
def refused(fm, mem, ranges, w, capacity):
    """the call fails with EINVAL and neither output holds anything but the fill"""
    r, keep = upload_ranges(mem, ranges)
    out, pout = mem.out(max(capacity, 1) * 8)
    off, poff = mem.out(8 * (len(r) + 1))
    msg = fc.einval(lambda: fm.extract(keep[0][1], keep[1][1], keep[2][1], len(r), w, pout, capacity, poff))
    assert bool(np.all(mem.get(out) == fc.FILL)) and bool(np.all(mem.get(off) == fc.FILL)), "a refused call wrote"
    return msg


def run_refusals(ctx, flags, mem, lib):
    col = wk.COLS["dna"]
    k = len(col.strings)
    idx = 8 if flags & engine.FLAG_FORCE_IDX64 else 4
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    fc.einval(lambda: engine.FmIndex(ctx, img, len(blob), locate=False, extract=True))
    fc.einval(lambda: engine.FmIndex(ctx, img, len(blob), locate=False, checkpoints=True, extract=True))
    for bits in (None, 4):
        with make_index(ctx, flags, mem, lib, col, bits) as fm, make_index(ctx, flags, mem, lib, col, bits, extract=False) as plain:
            Q = sample_positions(fm, mem, col, bits)
            ranges = [(s, 1, MAX) for s in range(k)]
            total = int((slens(col) - 1).sum())
            check(fm, mem, col, Q, ranges, on_gpu=mem.on_gpu)
            bad = list(ranges)
            bad[7] = (k, 0, 1)
            bad[9] = (MAX, 0, 1)
            msg = refused(fm, mem, bad, 1, total)
            assert "range 7 " in msg, msg
            assert "cells" in refused(fm, mem, ranges, 1, total - 1)
            refused(fm, mem, ranges, 3, total)
            refused(fm, mem, ranges, 0, total)
            refused(plain, mem, ranges, 1, total)
            ln, pl = mem.out(8 * k)
            fc.einval(lambda: plain.string_lengths(pl))
            assert bool(np.all(mem.get(ln) == fc.FILL))
            with __import__("pytest").raises(engine.GrlbwtError) as e:
                plain.extract_info()
            assert e.value.code == EINVAL
            # accounting: the bit adds extract_bytes, and nothing else changes
            a, b, xi = plain.info(), fm.info(), fm.extract_info()
            want = engine.FM_LOCATE | engine.FM_EXTRACT | (0 if bits is None else engine.FM_CHECKPOINTS | (bits << 8))
            assert b["flags"] == want and a["flags"] == want & ~engine.FM_EXTRACT
            assert b["index_bytes"] == a["index_bytes"] + xi["extract_bytes"]
            assert xi["extract_bytes"] == (2 * xi["n_samples"] + k + 1) * idx and xi["n_samples"] == len(Q)
            assert {q: v for q, v in a.items() if q not in ("flags", "index_bytes")} == {q: v for q, v in b.items() if q not in ("flags", "index_bytes")}
            if bits is None:
                assert xi["n_samples"] == k
            else:
                assert fm.walk_info() == plain.walk_info()
                assert xi["n_samples"] <= fm.walk_info()["n_checkpoints"]
            # a call that succeeds after refused ones, and n = 0
            check(fm, mem, col, Q, ranges, on_gpu=mem.on_gpu)
            cells, offs, got = run_extract(fm, mem, np.zeros((0, 3), dtype=np.uint64), 1, 0)
            assert got == 0 and offs.tolist() == [0]


# ------------------------------------------------------------------ 8: foreign images
FOREIGN = wk.FOREIGN
FOREIGN_BITS = (None, 1, 6)


def run_foreign(ctx, mem, c):
    """Where the locate index is made the extract index is made too and its whole strings, one after the other, are what
    invert_image returns for the image (these images have no text: the stated exception); where it is refused, so is this one."""
    blob = c.image()
    keep, img = mem.put(blob)
    w = wk.cell_width(c)
    made = 0
    for bits in FOREIGN_BITS:
        kw = {} if bits is None else dict(checkpoints=True, sample_bits=bits)
        try:
            with engine.FmIndex(ctx, img, len(blob), locate=True, **kw) as fm:
                k = fm.info()["n_strings"]
        except engine.GrlbwtError as e:
            assert e.code == EINVAL
            with __import__("pytest").raises(engine.GrlbwtError) as e2:
                engine.FmIndex(ctx, img, len(blob), locate=True, extract=True, **kw)
            assert e2.value.code == e.code, (c.name, bits)
            continue
        made += 1
        with engine.FmIndex(ctx, img, len(blob), locate=True, extract=True, **kw) as fm:
            assert fm.info()["n_strings"] == k
            try:
                text, pt = mem.out(c.n * w)
                n = ctx.invert_image(img, len(blob), w, pt, c.n)
                want = mem.body(text, c.n * w)[:n * w].view(DT[w])
            except engine.GrlbwtError:
                want = None                              # (rows on no string's chain: the inverter refuses, the index does not)
            ranges = [(s, 0, MAX) for s in range(k)]
            ln, pl = mem.out(8 * k)
            fm.string_lengths(pl)
            lens = mem.body(ln, 8 * k).view(np.uint64)
            total = int(lens.sum())
            assert total <= c.n
            cells, offs, got = run_extract(fm, mem, ranges, w, total)
            assert got == total and np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
            if want is not None:
                assert total == c.n and cells.tobytes() == want.tobytes(), c.name
            xi = fm.extract_info()
            assert xi["n_ranges"] == k and xi["n_cells"] == total
    return made
