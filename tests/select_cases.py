"""Shared by tests/test_image_select_sim.py (serial stand-in) and tests/test_image_select_gpu.py (HIP library): removing or
keeping chosen strings of an .rl_bwt image (grlbwt_select_*), against values that share no code with the feature.

  a  the image grlbwt_build makes of the text of the remaining strings (the path the parity suite pins), byte for byte
  b  for collections of at most 2000 cells also bcr_check.naive_rl_bwt of that text
  c  rows() against a numpy model: the rows of the listed strings' suffixes in the naive BCR suffix order; rows_marked is the sum
     of their lengths

Every case runs on a plain context and on one with 64-bit positions (the callers loop), every output buffer has guard bytes
behind it.  Engine-built images are built once per library and kept (merge_cases.build).
"""
import ctypes as C
import os

import numpy as np
import pytest

from grlbwt_amd import engine
from tests import bcr_check as bc
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import merge_cases as mc
from tests import walk_cases as wk

EINVAL = -22
DT = fc.DT
FILL = fc.FILL
ACGT = mc.ACGT
build = mc.build


# ------------------------------------------------------------------ collections and lists
def collection(name, strings, sep, w):
    return fc.Collection(name, mc.text(strings, sep, w), w)


def text_of(col, which):
    """the cells of the strings `which` (ascending numbers) of a collection"""
    return mc.text([col.strings[i] for i in which], col.sep, col.w)


def complement(k, ids):
    s = set(int(i) for i in ids)
    return [i for i in range(k) if i not in s]


def dna_lists():
    col = fc.COLS["dna"]
    k = len(col.strings)
    empty = [i for i, s in enumerate(col.strings) if len(s) == 0]
    seen, dup = {}, None
    for i, s in enumerate(col.strings):
        if len(s) and s.tobytes() in seen:
            dup = i
            break
        seen[s.tobytes()] = i
    assert empty and dup is not None and k == 300
    return {
        "first": [0],
        "last": [k - 1],
        "an_empty_string": [empty[0]],
        "one_of_a_duplicated_pair": [dup],
        "every_second": list(range(0, k, 2)),
        "all_but_one": complement(k, [17]),
        "repeats_descending": [250, 250, 199, 64, 64, 63, 5, 5, 5, 0],
    }


DNA_LISTS = dna_lists()


def edge_collections():
    """collections of exactly 63 .. 129 rows (the mark vector's last word) and of 63, 64 and 65 strings (the k-bit set)"""
    rng = np.random.default_rng(20261019)
    out = {}
    for n in (63, 64, 65, 127, 128, 129):
        out["rows_%d" % n] = collection("rows_%d" % n, mc.strings_to(rng, n, ACGT, 1, first=[ACGT[:0]]), 10, 1)
        assert out["rows_%d" % n].n == n
    out["strings_64"] = fc.COLS["identical"]
    for k in (63, 65):
        out["strings_%d" % k] = collection("strings_%d" % k, [ACGT[rng.integers(0, 4, size=int(rng.integers(0, 6)))] for _ in range(k)], 10, 1)
    return out


EDGES = edge_collections()
EDGE_NAMES = list(EDGES)


def header_collections():
    rng = np.random.default_rng(77)

    def rand(m):
        return ACGT[rng.integers(0, 4, size=m)]

    out = {}
    # the only symbols of 252 and above sit in strings 3 and 9: sb 2 -> 1
    strs = [rand(int(rng.integers(1, 30))) for _ in range(12)]
    strs[3] = np.concatenate([rand(5), [253], rand(4)]).astype(np.uint8)
    strs[9] = np.array([255, 252], dtype=np.uint8)
    out["sb_2_to_1"] = (collection("sb_2_to_1", strs, 10, 1), [3, 9])
    # the largest byte frequency falls from >= 256 to < 256 with string 0: fb 2 -> 1
    strs = [np.repeat(ACGT[:1], 250)] + [rand(10) for _ in range(20)]
    out["fb_2_to_1"] = (collection("fb_2_to_1", strs, 10, 1), [0])
    # two-byte cells: the length falls below 256
    pool = 300 + 7 * np.arange(40)
    strs = [pool[rng.integers(0, 40, size=10)] for _ in range(30)]
    out["two_byte_length_below_256"] = (collection("two_byte_length_below_256", strs, 3, 2), list(range(1, 30, 3)) + [29])
    return out


HEADERS = header_collections()


# ------------------------------------------------------------------ one selection
def ids_array(ids):
    return np.asarray(list(ids), dtype=np.uint64)


def select_bytes(ctx, mem, blob, w, ids, keep=False, checkpoints=False, sample_bits=0):
    """(image, info, marked rows as 0/1 per row) of one selection on an image given as bytes"""
    ids = ids_array(ids)
    ki, pi = mem.put(blob)
    kl, pl = mem.put(ids.tobytes())
    with engine.ImageSelect(ctx, pi, len(blob), w, pl, len(ids), keep, checkpoints, sample_bits) as sel:
        del ki, kl                                                 # the selection has copied what it needs
        info = sel.info()
        out, po = mem.out(info["out_bytes"])
        sel.emit(po, info["out_bytes"])
        got = mem.body(out, info["out_bytes"]).tobytes()
        n = info["n_syms_in"]
        nw = (n + 63) // 64
        bits, pb = mem.out(8 * nw)
        sel.rows(pb)
        words = mem.body(bits, 8 * nw)
        z = np.unpackbits(words, bitorder="little")
        assert not z[n:].any()
    return got, info, z[:n]


_rows = {}


def row_strings(col):
    """the string of every row: the naive BCR suffix order"""
    if col.name not in _rows:
        _rows[col.name] = (fc.dna_sa(col) if col.name == "dna" and col is fc.COLS["dna"] else wk.suffix_order(col))[0]
    return _rows[col.name]


def check_info(info, flags, col, listed, keep, got):
    k, n = len(col.strings), col.n
    listed = sorted(set(int(i) for i in listed))
    rest = listed if keep else complement(k, listed)
    marked = sum(len(col.strings[i]) + 1 for i in listed)
    n_out = marked if keep else n - marked
    sb, fb, sym, ln = bc.parse_rl_bwt(got)
    assert (info["n_syms_in"], info["n_strings_in"], info["n_listed"], info["rows_marked"]) == (n, k, len(listed), marked), info
    assert (info["n_syms_out"], info["n_strings_out"]) == (n_out, len(rest)), info
    assert (info["sb"], info["fb"], info["n_runs_out"], info["out_bytes"]) == (sb, fb, len(sym), len(got)), info
    assert info["n_runs_out"] <= info["n_runs_in"] and int(ln.sum()) == n_out
    assert bc.runs_are_maximal(sym) and int(ln.min()) > 0
    assert info["separator"] == col.sep and info["idx_bytes"] == (8 if flags & engine.FLAG_FORCE_IDX64 else 4)
    assert info["held_bytes"] >= n // 8 and info["scratch_bytes"] > 0
    if not info["flags"] & engine.SELECT_CHECKPOINTS:
        assert info["longest_walk"] == max([len(col.strings[i]) + 1 for i in listed], default=0)
        assert (info["sample_bits"], info["n_checkpoints"], info["jump_rounds"]) == (0, 0, 0)
        assert info["lane_refills"] == max(0, len(listed) - info["walk_lanes"]), info


def run_one(ctx, flags, mem, lib, col, ids, keep=False, rows_model=True, **kw):
    """one selection on the engine's image of a collection, against a, b and c; returns (bytes, info, rows)"""
    k = len(col.strings)
    listed = sorted(set(int(i) for i in ids))
    rest = listed if keep else complement(k, listed)
    want_text = text_of(col, rest)
    got, info, z = select_bytes(ctx, mem, build(lib, flags, col.data, col.w), col.w, ids, keep, **kw)
    assert got == build(lib, flags, want_text, col.w), (col.name, ids[:8], keep)            # (a)
    if len(want_text) <= 2000:
        assert got == bc.naive_rl_bwt(want_text.tobytes(), col.w), (col.name, ids[:8], keep)  # (b)
    if rows_model:
        assert np.array_equal(z, np.isin(row_strings(col), ids_array(listed)).astype(np.uint8)), (col.name, ids[:8])      # (c)
    check_info(info, flags, col, listed, keep, got)
    return got, info, z


# ------------------------------------------------------------------ 1: the DNA collection
def run_dna_list(ctx, flags, mem, lib, name):
    col = fc.COLS["dna"]
    ids = DNA_LISTS[name]
    k = len(col.strings)
    dropped, _, z_drop = run_one(ctx, flags, mem, lib, col, ids, keep=False)
    kept, _, z_keep = run_one(ctx, flags, mem, lib, col, ids, keep=True)
    assert np.array_equal(z_drop, z_keep)                           # the keep flag does not change the bits
    other, _, z_other = run_one(ctx, flags, mem, lib, col, complement(k, ids), keep=False)
    assert kept == other and np.array_equal(z_other, 1 - z_keep)    # keep S == drop (complement of S)
    assert dropped != kept


# ------------------------------------------------------------------ 2: word and wave edges
def run_edge(ctx, flags, mem, lib, name):
    col = EDGES[name]
    k = len(col.strings)
    assert k >= 3
    for ids in ([k - 1], [0, k - 1], list(range(1, k, 3)) + [k - 1]):
        for keep in (False, True):
            run_one(ctx, flags, mem, lib, col, ids, keep=keep)
    run_one(ctx, flags, mem, lib, col, list(range(1, k, 3)), checkpoints=True, sample_bits=2)


def run_lanes(ctx, flags, mem, lib):
    """130 listed strings (the caller sets the number of lanes to 64 on the device)"""
    col = fc.COLS["dna"]
    ids = list(range(3, 3 + 2 * 130, 2))
    _, info, _ = run_one(ctx, flags, mem, lib, col, ids)
    assert info["n_listed"] == 130
    if mem.on_gpu:
        assert info["walk_lanes"] == 64, info
    assert info["lane_refills"] == max(0, info["n_listed"] - info["walk_lanes"]), info
    return info


# ------------------------------------------------------------------ 3: header edges
def run_header(ctx, flags, mem, lib, name):
    col, ids = HEADERS[name]
    rest = text_of(col, complement(len(col.strings), ids))
    before, after = bc.header_widths(col.data, col.w), bc.header_widths(rest, col.w)
    if name == "sb_2_to_1":
        assert (before[0], after[0]) == (2, 1)
    else:
        assert (before[1], after[1]) == (2, 1), (before, after)
    got, info, _ = run_one(ctx, flags, mem, lib, col, ids)
    assert (info["sb"], info["fb"]) == after
    assert bc.parse_rl_bwt(build(lib, flags, col.data, col.w))[:2] == before


def run_runs_join(ctx, flags, mem, lib):
    """a removal after which runs of one symbol become neighbours: fewer runs than the emptied ones account for"""
    col = fc.COLS["dna"]
    ids = DNA_LISTS["every_second"]
    got, info, z = run_one(ctx, flags, mem, lib, col, ids)
    _, _, sym, ln = bc.parse_rl_bwt(build(lib, flags, col.data, col.w))
    ends = np.cumsum(ln.astype(np.int64))
    marked_in_run = np.add.reduceat(z.astype(np.int64), ends - ln.astype(np.int64))
    emptied = int((marked_in_run == ln.astype(np.int64)).sum())
    assert info["n_runs_in"] == len(sym) and emptied > 0
    assert info["n_runs_out"] < info["n_runs_in"] - emptied, (info["n_runs_out"], info["n_runs_in"], emptied)
    assert bc.runs_are_maximal(bc.parse_rl_bwt(got)[2])


# ------------------------------------------------------------------ 4: two-byte and wide symbols
def run_wide(ctx, flags, mem, lib, name):
    col = fc.COLS[name]
    k = len(col.strings)
    ids = list(range(0, k, 3))
    rest = text_of(col, complement(k, ids))
    got, info, _ = run_one(ctx, flags, mem, lib, col, ids, rows_model=col.n <= 20000)
    kg, pg = mem.put(got)
    out, po = mem.out(len(rest) * col.w)
    assert ctx.invert_image(pg, len(got), col.w, po, len(rest)) == len(rest)
    assert np.array_equal(mem.body(out, len(rest) * col.w).view(DT[col.w]), rest), name


# ------------------------------------------------------------------ 5: the checkpointed form
CP_BITS = (4, 6, 0)
_plain = {}


def cp_lists(col):
    k = len(col.strings)
    return [[i] for i in range(k)] + ([[0, 2]] if k > 2 else [])


def run_checkpointed(ctx, flags, mem, lib, name, bits):
    col = wk.COLS[name]
    blob = fc.image_of(lib, col, flags)
    k, n = len(col.strings), col.n
    for j, ids in enumerate(cp_lists(col)):
        key = (lib, flags, name, tuple(ids))
        if key not in _plain:
            _plain[key] = select_bytes(ctx, mem, blob, col.w, ids)
            got, info, _ = _plain[key]
            check_info(info, flags, col, ids, False, got)
            if j == 0:                                              # (a) once per collection: the others against this form
                assert got == build(lib, flags, text_of(col, complement(k, ids)), col.w), (name, ids)
        want, winfo, wz = _plain[key]
        got, info, z = select_bytes(ctx, mem, blob, col.w, ids, checkpoints=True, sample_bits=bits)
        assert got == want and np.array_equal(z, wz), (name, bits, ids)
        check_info(info, flags, col, ids, False, got)
        b = info["sample_bits"]
        assert (b == bits) if bits else (1 <= b <= 20), info
        assert info["n_checkpoints"] == k + -(-n // (1 << b)), info
        assert info["jump_rounds"] <= wk.ceil_log2(info["n_checkpoints"]) and info["longest_walk"] <= n
        assert info["flags"] == engine.select_flags(False, True, bits)


def run_checkpointed_dna(ctx, flags, mem, lib):
    col = fc.COLS["dna"]
    for keep in (False, True):
        run_one(ctx, flags, mem, lib, col, DNA_LISTS["every_second"], keep=keep, checkpoints=True, sample_bits=1)
    run_one(ctx, flags, mem, lib, col, DNA_LISTS["repeats_descending"], checkpoints=True, sample_bits=1)


# ------------------------------------------------------------------ 6: algebra with the merge
def run_merge_algebra(ctx, flags, mem, lib):
    rng = np.random.default_rng(31)
    a, b = mc.dna_pair(rng, 3000, 5200)
    ka, kb = int((a == 10).sum()), int((b == 10).sum())
    img_a, img_b, img_ab = build(lib, flags, a, 1), build(lib, flags, b, 1), build(lib, flags, np.concatenate([a, b]), 1)
    merged = mc.merge_bytes(ctx, mem, img_a, img_b, 1)[0]
    b_ids = list(range(ka, ka + kb))
    assert select_bytes(ctx, mem, merged, 1, b_ids)[0] == img_a
    assert select_bytes(ctx, mem, merged, 1, b_ids, keep=True)[0] == img_b
    a_ids = list(range(ka))
    first, second = select_bytes(ctx, mem, img_ab, 1, a_ids, keep=True)[0], select_bytes(ctx, mem, img_ab, 1, a_ids)[0]
    assert (first, second) == (img_a, img_b)
    assert mc.merge_bytes(ctx, mem, first, second, 1)[0] == img_ab


# ------------------------------------------------------------------ 7: foreign encodings
def outcome(ctx, mem, blob, w, ids, **kw):
    try:
        return select_bytes(ctx, mem, blob, w, ids, **kw)[0]
    except engine.GrlbwtError as e:
        assert e.code == EINVAL, e
        return EINVAL


def run_foreign(ctx, flags, mem, lib):
    col = fc.COLS["dna"]
    img = build(lib, flags, col.data, 1)
    ids = DNA_LISTS["repeats_descending"]
    want = build(lib, flags, text_of(col, complement(len(col.strings), ids)), 1)
    cut = mc.split_runs(ctx, mem, img, 2, 7)                        # empty records, equal neighbours, other widths
    _, _, sym, ln = bc.parse_rl_bwt(cut)
    assert int((ln == 0).sum()) > 0 and not bc.runs_are_maximal(sym) and len(cut) != len(img)
    _, _, sym, ln = bc.parse_rl_bwt(img)
    wide = ic.make_image(8, 8, sym, ln)                             # header widths (8, 8)
    for blob in (cut, wide):
        assert select_bytes(ctx, mem, blob, 1, ids)[0] == want
        assert select_bytes(ctx, mem, blob, 1, ids, checkpoints=True, sample_bits=3)[0] == want
        assert select_bytes(ctx, mem, blob, 1, [])[0] == img         # removing nothing: the canonical image
        assert select_bytes(ctx, mem, blob, 1, range(len(col.strings)), keep=True)[0] == img


FOREIGN = [c.name for c in ic.CASES if c.R >= 1 and not c.giant]


def run_not_a_collection(ctx, flags, mem, c):
    """images that are no BWT of a collection: GRLBWT_EINVAL or a result, the same from both marking forms"""
    blob = c.image()
    csym, clen = ic.canonical(c.syms, c.lens)
    k = int(clen[csym == csym.min()].sum()) if len(csym) else 0
    nothing = outcome(ctx, mem, blob, 8, [])
    if len(csym):
        _, _, sym, ln = bc.parse_rl_bwt(nothing)
        assert np.array_equal(sym, csym) and np.array_equal(ln, clen), c.name
    else:
        assert nothing == EINVAL
    for ids in ([0], [k - 1, 0] if k else [0], list(range(0, k, 2))):
        one = outcome(ctx, mem, blob, 8, ids)
        two = outcome(ctx, mem, blob, 8, ids, checkpoints=True, sample_bits=2)
        assert one == two, (c.name, ids)
        if k == 0 or len(set(ids)) >= k:
            assert one == EINVAL, (c.name, ids)
        else:
            assert one != EINVAL, (c.name, ids)
            _, _, sym, ln = bc.parse_rl_bwt(one)
            assert bc.runs_are_maximal(sym) and int(ln.min()) > 0


# ------------------------------------------------------------------ 8: refusals
def create_raw(ctx, pi, nbytes, w, pl, n_ids, sflags):
    """grlbwt_select_create itself: (return code, *out, message) with *out preset to a value that is no handle"""
    h = C.c_void_p(0xDEAD0)
    rc = ctx.L.grlbwt_select_create(ctx._h, C.c_void_p(pi), nbytes, w, C.c_void_p(pl), n_ids, sflags, C.byref(h))
    if rc == 0:
        ctx.L.grlbwt_select_destroy(ctx._h, h)
    return rc, h.value, ctx.L.grlbwt_last_error(ctx._h).decode()


def refused(ctx, mem, blob, w, ids, sflags=0, code=EINVAL):
    ids = ids_array(ids)
    ki, pi = mem.put(blob)
    kl, pl = mem.put(ids.tobytes())
    rc, h, msg = create_raw(ctx, pi, len(blob), w, pl, len(ids), sflags)
    assert (rc, h) == (code, None), (rc, h, msg)
    return msg


def run_refusals(ctx, flags, mem, lib):
    col = fc.COLS["dna"]
    k = len(col.strings)
    img = build(lib, flags, col.data, 1)
    msg = refused(ctx, mem, img, 1, [3, k, 5])                      # an id that is no string; the message names its position
    assert "entry 1 " in msg and str(k) in msg, msg
    msg = refused(ctx, mem, img, 1, [3, 4, 7, 2 ** 64 - 1, 5, k])
    assert "entry 3 " in msg and str(2 ** 64 - 1) in msg, msg
    refused(ctx, mem, img, 1, range(k))                             # everything removed
    refused(ctx, mem, img, 1, [], engine.SELECT_KEEP)               # keep of nothing
    refused(ctx, mem, img, 3, [0])                                  # cell_bytes
    two = fc.COLS["two_bytes"]
    assert int(two.data.max()) > 255
    refused(ctx, mem, build(lib, flags, two.data, 2), 1, [0])       # a symbol that does not fit one byte
    for sflags in (4 << 8, engine.SELECT_CHECKPOINTS | (21 << 8), 4, 1 << 16, 1 << 31):
        msg = refused(ctx, mem, img, 1, [0], sflags)                # sample_bits without the flag, above 20, unknown bits
        assert "GRLBWT_" not in msg
    refused(ctx, mem, ic.make_image(1, 2, [], []), 1, [0])          # a 16-byte image
    refused(ctx, mem, img[:-1], 1, [0])                             # a bad header
    # emit into a buffer one byte short: nothing is written
    ids = ids_array(DNA_LISTS["every_second"])
    ki, pi = mem.put(img)
    kl, pl = mem.put(ids.tobytes())
    with engine.ImageSelect(ctx, pi, len(img), 1, pl, len(ids)) as sel:
        nbytes = sel.info()["out_bytes"]
        out, po = mem.out(nbytes)
        with pytest.raises(engine.GrlbwtError) as e:
            sel.emit(po, nbytes - 1)
        assert e.value.code == EINVAL
        assert bool(np.all(mem.get(out) == FILL))
        sel.emit(po, nbytes)
        assert mem.body(out, nbytes).tobytes() == build(lib, flags, text_of(col, complement(k, ids)), 1)


# ------------------------------------------------------------------ 9: handles and their context
def run_handles_outlive_the_context(mem, lib):
    """grlbwt_ctx_destroy releases the selections still alive; closing such a selection afterwards touches nothing."""
    col = fc.COLS["dna"]
    img = build(lib, 0, col.data, 1)
    ids = ids_array([1, 2, 3])
    ki, pi = mem.put(img)
    kl, pl = mem.put(ids.tobytes())
    ctx = engine.Context(0, 0, lib)
    one = engine.ImageSelect(ctx, pi, len(img), 1, pl, len(ids))
    two = engine.ImageSelect(ctx, pi, len(img), 1, pl, len(ids), keep=True)
    assert one.info()["n_listed"] == 3
    two.close()
    ctx.close()
    one.close()
    one.close()
    with engine.Context(0, 0, lib) as ctx2:                         # the library is as it was
        assert select_bytes(ctx2, mem, img, 1, ids)[0] == build(lib, 0, text_of(col, complement(len(col.strings), ids)), 1)


# ------------------------------------------------------------------ 10: files
def run_files(ctx, flags, mem, lib, tmp_path):
    col = fc.COLS["dna"]
    k = len(col.strings)
    ids = DNA_LISTS["every_second"]
    pin, pout, pwant = (str(tmp_path / n) for n in ("in.rl_bwt", "out.rl_bwt", "built.rl_bwt"))
    open(pin, "wb").write(build(lib, flags, col.data, 1))
    with engine.Context(0, flags, lib) as c2:
        c2.upload(text_of(col, complement(k, ids)).tobytes(), 1)
        c2.build()
        c2.write_file(pwant)
    want = open(pwant, "rb").read()
    open(pout, "wb").write(want + b"tail of an older, longer file" * 10)
    info = ctx.select_files(pin, ids, pout, 1)
    assert open(pout, "rb").read() == want                          # (a), and no tail of the file that was there
    assert info["out_bytes"] == os.path.getsize(pout) and info["n_listed"] == len(ids)
    info = ctx.select_files(pin, complement(k, ids), pout, 1, keep=True, checkpoints=True, sample_bits=4)
    assert open(pout, "rb").read() == want and info["n_checkpoints"] > k
    os.remove(pout)
    with pytest.raises(engine.GrlbwtError) as e:                    # an error code, no exception across the ABI, no file
        ctx.select_files(pin, [k], pout, 1)
    assert e.value.code == EINVAL and not os.path.exists(pout)
    with pytest.raises(engine.GrlbwtError) as e:
        ctx.select_files(str(tmp_path / "missing.rl_bwt"), [0], pout, 1)
    assert e.value.code < 0 and not os.path.exists(pout)
