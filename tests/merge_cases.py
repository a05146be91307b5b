"""Shared by tests/test_image_merge_sim.py (serial stand-in) and tests/test_image_merge_gpu.py (HIP library): merging two
.rl_bwt images (grlbwt_merge_*) into the image of "A's strings, then B's", against values that share no code with the merge.

  a  for every pair the image grlbwt_build makes of the concatenated text (the path the parity suite pins), byte for byte
  b  for pairs of at most 2000 cells also bcr_check.naive_rl_bwt of the concatenation
  c  the interleave and the number of rounds from a numpy model of the definition (model below: a stable argsort per round,
     the separator's bucket rewritten); the rows picked through grlbwt_merge_interleave's bits must give the decoded image

The inputs are sized from the tile the library reports (info()["tile_rows"] of a first tiny merge), never from a constant:
merged row counts around one tile and over three, slices that leave whole tiles to one image, one bucket, 256 buckets.
Every output buffer has guard bytes behind it.  Engine-built images are built once per library and kept.
"""
import ctypes as C
import os

import numpy as np
import pytest

from grlbwt_amd import engine
from tests import bcr_check as bc
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import wide_check as wc

EINVAL, ERANGE = -22, -75
DT = fc.DT
FILL = fc.FILL
HERE = os.path.dirname(os.path.abspath(__file__))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ------------------------------------------------------------------ collections
def text(strings, sep, w):
    """strings (arrays without their separator) -> the cells of the collection"""
    parts = []
    for s in strings:
        parts += [np.asarray(s, dtype=DT[w]), np.array([sep], dtype=DT[w])]
    return np.concatenate(parts).astype(DT[w])


def strings_to(rng, total, pool, w, first=()):
    """strings of 1 to 60 cells over `pool` (after `first`) whose collection has exactly `total` cells, separators included"""
    out = [np.asarray(s, dtype=DT[w]) for s in first]
    left = total - sum(len(s) + 1 for s in out)
    assert left >= 1
    while left > 61:
        m = int(rng.integers(1, 61))
        out.append(np.asarray(pool, dtype=DT[w])[rng.integers(0, len(pool), size=m)])
        left -= m + 1
    out.append(np.asarray(pool, dtype=DT[w])[rng.integers(0, len(pool), size=left - 1)])
    return out


def dna_pair(rng, n_a, n_b):
    """two DNA batches of exactly n_a and n_b cells: a few empty strings in each, a few strings of A again in B"""
    empty = ACGT[:0]
    a = strings_to(rng, n_a, ACGT, 1, first=[empty] if n_a > 200 else [])
    shared = [a[int(rng.integers(len(a)))] for _ in range(3)] if n_b > 400 else []
    b = strings_to(rng, n_b, ACGT, 1, first=shared + ([empty, empty] if n_b > 200 else []))
    order = rng.permutation(len(b))
    return text(a, 10, 1), text([b[i] for i in order], 10, 1)


class Pair:
    def __init__(self, name, a, b, w):
        self.name, self.a, self.b, self.w = name, np.asarray(a, dtype=DT[w]), np.asarray(b, dtype=DT[w]), w
        self.ab = np.concatenate([self.a, self.b])
        self.sep = int(self.ab[-1])
        assert int(self.a[-1]) == self.sep and int(self.ab.min()) == self.sep
        self.n = len(self.ab)


def make_pairs(T):
    """the pairs, sized by the tile T of the round kernels"""
    rng = np.random.default_rng(20261019)
    P = []
    for n in (T - 1, T, T + 1, 3 * T + 17):                       # merged rows around one tile and over three
        na = n // 2 - 5
        P.append(Pair("rows_%s" % {T - 1: "tile_minus_1", T: "tile", T + 1: "tile_plus_1"}.get(n, "three_tiles_17"), *dna_pair(rng, na, n - na), 1))
    one = text([ACGT[rng.integers(0, 4, size=37)]], 10, 1)
    big = text(strings_to(rng, 2 * T + 9, ACGT, 1), 10, 1)
    P.append(Pair("one_string_against_two_tiles", one, big, 1))
    P.append(Pair("two_tiles_against_one_string", big, one, 1))
    lo = text(strings_to(rng, T + T // 2 + 3, ACGT[:2], 1), 10, 1)        # A over {A, C}, B over {G, T}: B's suffixes sort above A's,
    hi = text(strings_to(rng, T + T // 2 - 7, ACGT[2:], 1), 10, 1)        # whole tiles come from one image, the slice starts take every alignment
    P.append(Pair("disjoint_alphabets", lo, hi, 1))
    P.append(Pair("one_symbol", text(strings_to(rng, T // 2 + 3, ACGT[:1], 1), 10, 1), text(strings_to(rng, T // 2 + 40, ACGT[:1], 1), 10, 1), 1))
    raw = np.frombuffer(open(os.path.join(HERE, "golden", "test_2bytes_alphabet.txt"), "rb").read(), dtype=np.uint16)
    if len(np.unique(raw)) <= 256:                                  # the golden collection, cut at a string boundary
        ends = np.flatnonzero(raw == raw[-1])
        cut = int(ends[len(ends) // 2]) + 1
        P.append(Pair("two_bytes", raw[:cut], raw[cut:], 2))
    else:                                                           # (it has more: a seeded 2-byte collection of 200 distinct values)
        pool = 300 + 7 * np.arange(199)
        P.append(Pair("two_bytes", text(strings_to(rng, 1500, pool, 2), 3, 2), text(strings_to(rng, 1100, pool, 2), 3, 2), 2))
    wa = wc.collection(rng, 8, 30, 40, 40, 2 ** 30 - 3, 2 ** 63)
    vals = np.unique(wa)
    wb = text(strings_to(rng, 600, vals[1:], 8), int(vals[0]), 8)
    P.append(Pair("wide_u64", wa, wb, 8))
    pool = 1000 + 3 * np.arange(255)                                # 255 values and the separator: exactly 256, accepted
    P.append(Pair("sigma_256", text([pool[:60], pool[60:120], pool[120:128]] + strings_to(rng, 900, pool, 2), 5, 2),
                  text([pool[128:188], pool[188:248], pool[248:]] + strings_to(rng, 700, pool, 2), 5, 2), 2))
    x = fc.COLS["identical"].data                                   # merge(X, X): every tie falls A first
    P.append(Pair("identical", x, x, 1))
    return P


_pairs = {}


def pairs(T):
    if T not in _pairs:
        _pairs[T] = {p.name: p for p in make_pairs(T)}
    return _pairs[T]


PAIR_NAMES = ["rows_tile_minus_1", "rows_tile", "rows_tile_plus_1", "rows_three_tiles_17", "one_string_against_two_tiles",
              "two_tiles_against_one_string", "disjoint_alphabets", "one_symbol", "two_bytes", "wide_u64", "sigma_256", "identical"]


# ------------------------------------------------------------------ expected values
_built = {}


def build(lib, flags, cells, w):
    """the image grlbwt_build makes of the cells (kept per library)"""
    cells = np.asarray(cells, dtype=DT[w])
    key = (lib, flags, w, cells.tobytes())
    if key not in _built:
        with engine.Context(0, flags, lib) as ctx:
            ctx.upload(cells.tobytes(), w)
            ctx.build()
            _built[key] = ctx.result_bytes()
    return _built[key]


def decode(blob):
    _, _, sym, ln = bc.parse_rl_bwt(blob)
    return ic.decode(sym, ln)


def model(bwt_a, bwt_b, sep):
    """The definition: Z = 0^nA 1^nB; a round reads the merged symbols through Z, moves every row's flag where a stable sort by
    the symbol puts it and rewrites the separator's bucket to 0^kA 1^kB; the round that changes nothing is the last one.
    Returns (Z, rounds)."""
    na, nb = len(bwt_a), len(bwt_b)
    ka, kb = int(np.count_nonzero(bwt_a == sep)), int(np.count_nonzero(bwt_b == sep))
    z = np.concatenate([np.zeros(na, dtype=np.uint8), np.ones(nb, dtype=np.uint8)])
    rounds = 0
    while True:
        sym = np.empty(na + nb, dtype=np.uint64)
        sym[z == 0] = bwt_a
        sym[z == 1] = bwt_b
        z2 = z[np.argsort(sym, kind="stable")]
        z2[:ka] = 0
        z2[ka:ka + kb] = 1
        rounds += 1
        if np.array_equal(z2, z):
            return z, rounds
        z = z2


_models = {}


def tile_rows(ctx, mem, lib, flags):
    """the tile of the round kernels, from a first tiny merge"""
    blob = build(lib, flags, np.frombuffer(b"AC\nA\n", dtype=np.uint8), 1)
    k, p = mem.put(blob)
    with engine.ImageMerge(ctx, p, len(blob), p, len(blob), 1) as mg:
        t = mg.info()["tile_rows"]
    assert t >= 64
    return t


# ------------------------------------------------------------------ one merge, checked
def merge_bytes(ctx, mem, blob_a, blob_b, w, max_rounds=0):
    """(merged image, info, interleave flags) of two images given as bytes"""
    ka, pa = mem.put(blob_a)
    kb, pb = mem.put(blob_b)
    with engine.ImageMerge(ctx, pa, len(blob_a), pb, len(blob_b), w, max_rounds) as mg:
        del ka, kb                                                 # the merge has copied what it needs
        info = mg.info()
        out, po = mem.out(info["out_bytes"])
        mg.emit(po, info["out_bytes"])
        got = mem.body(out, info["out_bytes"]).tobytes()
        n = info["n_syms_a"] + info["n_syms_b"]
        nw = (n + 63) // 64
        bits, pbits = mem.out(8 * nw)
        mg.interleave(pbits)
        words = mem.body(bits, 8 * nw).view(np.uint64)
        z = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
        assert not np.unpackbits(words.view(np.uint8), bitorder="little")[n:].any()
    return got, info, z


def run_pair(ctx, flags, mem, lib, name):
    T = tile_rows(ctx, mem, lib, flags)
    p = pairs(T)[name]
    img_a, img_b, want = build(lib, flags, p.a, p.w), build(lib, flags, p.b, p.w), build(lib, flags, p.ab, p.w)
    got, info, z = merge_bytes(ctx, mem, img_a, img_b, p.w)
    assert got == want, name                                        # (a)
    if p.n <= 2000:
        assert got == bc.naive_rl_bwt(p.ab.tobytes(), p.w), name    # (b)
    bwt_a, bwt_b = decode(img_a), decode(img_b)
    if (T, name) not in _models:
        _models[(T, name)] = model(bwt_a, bwt_b, p.sep)
    mz, mrounds = _models[(T, name)]
    assert info["rounds"] == mrounds and np.array_equal(z, mz), (name, info["rounds"], mrounds)        # (c)
    merged = np.empty(p.n, dtype=np.uint64)
    merged[z == 0] = bwt_a
    merged[z == 1] = bwt_b
    assert np.array_equal(merged, decode(want)), name
    sb, fb, sym, ln = bc.parse_rl_bwt(got)
    assert (info["sb"], info["fb"], info["n_runs"], info["out_bytes"]) == (sb, fb, len(sym), len(got))
    assert bc.runs_are_maximal(sym) and int(ln.min()) > 0
    assert (info["n_syms_a"], info["n_syms_b"], info["separator"], info["sigma"]) == (len(p.a), len(p.b), p.sep, len(np.unique(p.ab)))
    assert (info["n_strings_a"], info["n_strings_b"]) == (int((p.a == p.sep).sum()), int((p.b == p.sep).sum()))
    assert info["idx_bytes"] == (8 if flags & engine.FLAG_FORCE_IDX64 else 4) and info["tile_rows"] == T
    assert info["rows_changed"] >= (1 if mrounds > 1 else 0) and info["held_bytes"] >= 2 * p.n and info["scratch_bytes"] >= p.n
    return info


def run_sizes_follow_the_tile(ctx, flags, mem, lib):
    T = tile_rows(ctx, mem, lib, flags)
    P = pairs(T)
    assert [P[n].n for n in PAIR_NAMES[:4]] == [T - 1, T, T + 1, 3 * T + 17]
    assert P["one_string_against_two_tiles"].n > 2 * T and len(P["one_string_against_two_tiles"].a) < 64
    assert len(np.unique(P["sigma_256"].ab)) == 256 and len(np.unique(P["one_symbol"].ab)) == 2
    assert int(P["wide_u64"].ab.max()) == 2 ** 63 and len(np.unique(P["wide_u64"].ab)) <= 40
    for p in P.values():                                            # strings of at most 60 cells
        ends = np.flatnonzero(p.ab == p.sep)
        assert int(np.diff(np.concatenate([[-1], ends])).max()) <= 61, p.name


# ------------------------------------------------------------------ foreign encodings
def split_runs(ctx, mem, blob, bits, block):
    sb, _, sym, ln = bc.parse_rl_bwt(blob)
    n = int(ln.sum())
    cap = 16 + (len(sym) + n + n // block + 8) * (sb + 1)
    k, p = mem.put(blob)
    out, po = mem.out(cap)
    si = ctx.image_split_runs(p, len(blob), bits, block, po, cap)
    return mem.body(out, cap)[:si["out_bytes"]].tobytes()


def run_foreign(ctx, flags, mem, lib):
    T = tile_rows(ctx, mem, lib, flags)
    p = pairs(T)["rows_tile_plus_1"]
    img_a, img_b, want = build(lib, flags, p.a, p.w), build(lib, flags, p.b, p.w), build(lib, flags, p.ab, p.w)
    cut = split_runs(ctx, mem, img_a, 2, 7)                         # empty records, equal neighbours, other widths
    _, _, sym, ln = bc.parse_rl_bwt(cut)
    assert int((ln == 0).sum()) > 0 and not bc.runs_are_maximal(sym) and len(cut) != len(img_a)
    assert merge_bytes(ctx, mem, cut, img_b, p.w)[0] == want
    assert merge_bytes(ctx, mem, img_b, cut, p.w)[0] == build(lib, flags, np.concatenate([p.b, p.a]), p.w)
    _, _, sym, ln = bc.parse_rl_bwt(img_b)
    wide = ic.make_image(8, 8, sym, ln)                             # header widths (8, 8)
    assert merge_bytes(ctx, mem, cut, wide, p.w)[0] == want
    assert merge_bytes(ctx, mem, img_a, wide, p.w)[0] == want


# ------------------------------------------------------------------ associativity, round trip, max_rounds
def run_associativity(ctx, flags, mem, lib):
    rng = np.random.default_rng(77)
    a, b = dna_pair(rng, 600, 800)
    c = text(strings_to(rng, 500, ACGT, 1, first=[a[:0], b[:30][b[:30] != 10]]), 10, 1)
    ia, ib_, ic_ = (build(lib, flags, x, 1) for x in (a, b, c))
    left = merge_bytes(ctx, mem, merge_bytes(ctx, mem, ia, ib_, 1)[0], ic_, 1)[0]
    right = merge_bytes(ctx, mem, ia, merge_bytes(ctx, mem, ib_, ic_, 1)[0], 1)[0]
    assert left == right == build(lib, flags, np.concatenate([a, b, c]), 1)
    assert left == bc.naive_rl_bwt(np.concatenate([a, b, c]).tobytes(), 1)


def run_round_trip(ctx, flags, mem, lib, name):
    T = tile_rows(ctx, mem, lib, flags)
    p = pairs(T)[name]
    got = merge_bytes(ctx, mem, build(lib, flags, p.a, p.w), build(lib, flags, p.b, p.w), p.w)[0]
    k, pi = mem.put(got)
    out, po = mem.out(p.n * p.w)
    assert ctx.invert_image(pi, len(got), p.w, po, p.n) == p.n
    assert np.array_equal(mem.body(out, p.n * p.w).view(DT[p.w]), p.ab), name


def create_raw(ctx, pa, la, pb, lb, w, max_rounds=0):
    """grlbwt_merge_create itself: (return code, *out) with *out preset to a value that is no handle"""
    h = C.c_void_p(0xDEAD0)
    rc = ctx.L.grlbwt_merge_create(ctx._h, C.c_void_p(pa), la, C.c_void_p(pb), lb, w, max_rounds, C.byref(h))
    if rc == 0:
        ctx.L.grlbwt_merge_destroy(ctx._h, h)
    return rc, h.value


def run_max_rounds(ctx, flags, mem, lib):
    T = tile_rows(ctx, mem, lib, flags)
    p = pairs(T)["rows_tile"]
    img_a, img_b = build(lib, flags, p.a, p.w), build(lib, flags, p.b, p.w)
    free, info, _ = merge_bytes(ctx, mem, img_a, img_b, p.w)
    R = info["rounds"]
    assert R >= 3
    capped, info2, _ = merge_bytes(ctx, mem, img_a, img_b, p.w, R)
    assert capped == free and info2["rounds"] == R
    ka, pa = mem.put(img_a)
    kb, pb = mem.put(img_b)
    rc, h = create_raw(ctx, pa, len(img_a), pb, len(img_b), p.w, R - 1)
    assert (rc, h) == (EINVAL, None)
    msg = ctx.L.grlbwt_last_error(ctx._h).decode()
    assert "not converged" in msg and "max_rounds" in msg and "locate" in msg, msg


# ------------------------------------------------------------------ refusals
def refused(ctx, mem, blob_a, blob_b, w, code):
    ka, pa = mem.put(blob_a)
    kb, pb = mem.put(blob_b)
    rc, h = create_raw(ctx, pa, len(blob_a), pb, len(blob_b), w)
    assert (rc, h) == (code, None), (rc, h, ctx.L.grlbwt_last_error(ctx._h).decode())
    return ctx.L.grlbwt_last_error(ctx._h).decode()


def run_refusals(ctx, flags, mem, lib):
    rng = np.random.default_rng(5)
    a, b = dna_pair(rng, 300, 500)
    img_a, img_b = build(lib, flags, a, 1), build(lib, flags, b, 1)
    none = ic.make_image(1, 2, [], [])
    refused(ctx, mem, none, img_b, 1, EINVAL)                       # a 16-byte image on either side
    refused(ctx, mem, img_a, none, 1, EINVAL)
    refused(ctx, mem, img_a[:-1], img_b, 1, EINVAL)                 # a bad header: the size is no multiple of the record
    refused(ctx, mem, (9).to_bytes(8, "little") + img_a[8:], img_b, 1, EINVAL)
    zero = build(lib, flags, np.where(b == 10, 0, b), 1)            # separators 10 and 0
    msg = refused(ctx, mem, img_a, zero, 1, EINVAL)
    assert "10" in msg and "0 in B" in msg, msg
    refused(ctx, mem, img_a, img_b, 3, EINVAL)                      # cell_bytes
    w2 = text(strings_to(rng, 200, [65, 256], 2), 10, 2)
    refused(ctx, mem, img_a, build(lib, flags, w2, 2), 1, EINVAL)   # a symbol of 256 does not fit one byte
    pool = 1000 + 3 * np.arange(256)                                # 256 values and the separator: 257 distinct
    big_a, big_b = text([pool[:128]] + strings_to(rng, 300, pool, 2), 5, 2), text([pool[128:]] + strings_to(rng, 300, pool, 2), 5, 2)
    assert len(np.unique(np.concatenate([big_a, big_b]))) == 257
    msg = refused(ctx, mem, build(lib, flags, big_a, 2), build(lib, flags, big_b, 2), 2, ERANGE)
    assert "257" in msg and "256" in msg, msg
    # emit into a buffer one byte short: nothing is written
    ka, pa = mem.put(img_a)
    kb, pb = mem.put(img_b)
    with engine.ImageMerge(ctx, pa, len(img_a), pb, len(img_b), 1) as mg:
        nbytes = mg.info()["out_bytes"]
        out, po = mem.out(nbytes)
        with pytest.raises(engine.GrlbwtError) as e:
            mg.emit(po, nbytes - 1)
        assert e.value.code == EINVAL
        assert bool(np.all(mem.get(out) == FILL))
        mg.emit(po, nbytes)
        assert mem.body(out, nbytes).tobytes() == build(lib, flags, np.concatenate([a, b]), 1)


def run_handles_outlive_the_context(mem, lib):
    """grlbwt_ctx_destroy releases the merges still alive; closing such a merge afterwards touches nothing."""
    rng = np.random.default_rng(6)
    a, b = dna_pair(rng, 300, 500)
    img_a, img_b = build(lib, 0, a, 1), build(lib, 0, b, 1)
    ka, pa = mem.put(img_a)
    kb, pb = mem.put(img_b)
    ctx = engine.Context(0, 0, lib)
    one = engine.ImageMerge(ctx, pa, len(img_a), pb, len(img_b), 1)
    two = engine.ImageMerge(ctx, pb, len(img_b), pa, len(img_a), 1)
    assert one.info()["n_syms_a"] == len(a)
    two.close()
    ctx.close()
    one.close()
    one.close()
    with engine.Context(0, 0, lib) as ctx2:                         # the library is as it was
        assert merge_bytes(ctx2, mem, img_a, img_b, 1)[0] == build(lib, 0, np.concatenate([a, b]), 1)


# ------------------------------------------------------------------ files
def run_files(ctx, flags, mem, lib, tmp_path):
    rng = np.random.default_rng(8)
    a, b = dna_pair(rng, 900, 1300)
    pa, pb, pout, pwant = (str(tmp_path / n) for n in ("a.rl_bwt", "b.rl_bwt", "merged.rl_bwt", "built.rl_bwt"))
    open(pa, "wb").write(build(lib, flags, a, 1))
    open(pb, "wb").write(build(lib, flags, b, 1))
    with engine.Context(0, flags, lib) as c2:
        c2.upload(np.concatenate([a, b]).tobytes(), 1)
        c2.build()
        c2.write_file(pwant)
    info = ctx.merge_files(pa, pb, pout, 1)
    assert open(pout, "rb").read() == open(pwant, "rb").read()
    assert info["out_bytes"] == os.path.getsize(pout) and info["n_syms_a"] == len(a)
    os.remove(pout)
    with pytest.raises(engine.GrlbwtError) as e:                    # an error code, no exception across the ABI
        ctx.merge_files(pa, str(tmp_path / "missing.rl_bwt"), pout, 1)
    assert e.value.code < 0 and not os.path.exists(pout)
