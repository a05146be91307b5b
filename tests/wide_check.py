"""Shared by the wide-alphabet tests (CPU stand-in and GPU): expected bytes for collections whose symbols are 2^30 and larger,
from yardsticks that are not the code under test.

The oracle allocates max_sym + 1 bytes, so it is never called on the values: it is called on the RANK text
(np.unique's inverse, 8-byte cells), its run symbols are mapped back through the sorted values and re-encoded with the
header widths of the original cells."""
import json
import os

import numpy as np

from grlbwt_amd import engine
from oracle import oracle
from tests import bcr_check as bc
from tests import parity

DT = {4: np.uint32, 8: np.uint64}
ERANGE, EINVAL = -75, -22


def encode_np(sym, ln, sb, fb):
    sym = np.asarray(sym, dtype=np.uint64)
    ln = np.asarray(ln, dtype=np.uint64)
    rec = np.zeros((len(sym), sb + fb), dtype=np.uint8)
    for b in range(sb):
        rec[:, b] = ((sym >> np.uint64(8 * b)) & np.uint64(255)).astype(np.uint8)
    for b in range(fb):
        rec[:, sb + b] = ((ln >> np.uint64(8 * b)) & np.uint64(255)).astype(np.uint8)
    return int(sb).to_bytes(8, "little") + int(fb).to_bytes(8, "little") + rec.tobytes()


def ranks_of(cells):
    u, inv = np.unique(cells, return_inverse=True)
    return u.astype(np.uint64), inv.reshape(-1).astype(np.uint64)


def remap_image(rank_blob, values, cells, w):
    """The image of the rank text -> the image of the collection: symbols through `values`, header widths of the cells."""
    _, _, sym, ln = bc.parse_rl_bwt(rank_blob)
    sb, fb = bc.header_widths(cells, w)
    return encode_np(values[sym.astype(np.int64)], ln, sb, fb)


def oracle_on_ranks(cells, w):
    u, inv = ranks_of(cells)
    return remap_image(oracle.rl_bwt(inv.tobytes(), 8), u, cells, w)


def collection(rng, w, n_strings, max_len, n_distinct, lo, hi):
    """n_strings strings (empty ones and repeated ones among them) over n_distinct values of [lo, hi]; lo and hi occur."""
    span = hi - lo
    pool = sorted(set([lo, hi] + [lo + int(x) % (span + 1) for x in rng.integers(0, 2 ** 62, size=max(n_distinct - 2, 0))]))
    sep, body = pool[0], np.array(pool[1:], dtype=DT[w])
    strings = []
    for k in range(n_strings):
        r = rng.random()
        if r < 0.1:
            strings.append(np.zeros(0, dtype=DT[w]))
        elif r < 0.25 and strings:
            strings.append(strings[int(rng.integers(0, len(strings)))])
        else:
            strings.append(body[rng.integers(0, len(body), size=int(rng.integers(1, max_len + 1)))])
    strings.append(np.array([hi], dtype=DT[w]))
    parts = []
    for s in strings:
        parts += [s, np.array([sep], dtype=DT[w])]
    return np.concatenate(parts).astype(DT[w])


# (name, w, n_strings, max_len, n_distinct, lo, hi): few and many distinct values, around every width boundary
CASES = [
    ("u32_few_2^30", 4, 12, 20, 5, 2 ** 30 - 8, 2 ** 30 + 9),
    ("u32_many_full", 4, 40, 60, 900, 3, 2 ** 32 - 1),
    ("u32_top", 4, 25, 30, 40, 2 ** 32 - 100, 2 ** 32 - 1),
    ("u64_few_2^40", 8, 12, 20, 6, 2 ** 40 - 3, 2 ** 40 + 2 ** 33),
    ("u64_many_sparse", 8, 40, 60, 1200, 1, 2 ** 64 - 5),
    ("u64_2^63", 8, 25, 30, 50, 2 ** 63 - 20, 2 ** 63 + 20),
    ("u64_top", 8, 30, 25, 30, 2 ** 64 - 70, 2 ** 64 - 5),
    ("u64_low32_only", 8, 20, 30, 60, 2 ** 50, 2 ** 50 + 2 ** 31),
]
SMALL = [
    ("u32_small", 4, 5, 8, 6, 2 ** 31, 2 ** 31 + 50),
    ("u64_small", 8, 6, 7, 7, 2 ** 62, 2 ** 64 - 5),
]


def build_image(lib, cells, w, flags=0):
    with engine.Context(0, flags, lib) as ctx:
        ctx.upload(cells.tobytes(), w)
        st = ctx.stats()
        sigma = ctx.alphabet_size()
        values = ctx.alphabet_download() if sigma else None
        ctx.build()
        return ctx.result_bytes(), st, values


def check_final(lib, cells, w, flags=0):
    got, st, values = build_image(lib, cells, w, flags)
    u = np.unique(cells).astype(np.uint64)
    assert values is not None and np.array_equal(values, u), "alphabet_download() differs from np.unique"
    sb, fb = bc.header_widths(cells, w)
    assert (st["sb"], st["fb"], st["min_sym"], st["max_sym"], st["n_syms"]) == (sb, fb, int(cells.min()), int(cells.max()), len(cells))
    exp = oracle_on_ranks(cells, w)
    assert got == exp, "rl_bwt differs from the oracle on ranks (%d vs %d bytes)" % (len(got), len(exp))
    return got


def golden_cases():
    fx = json.load(open(os.path.join(parity.GOLD, "wide_alphabet.json")))
    return fx["cases"]


def ref_stats_edge():
    fx = json.load(open(os.path.join(parity.GOLD, "ref_stats.json")))
    return [c for c in fx["cases"] if c["name"] == "edge:max_sym=4294967295,w=4"][0]


def check_reference_case(lib, c):
    """stats and header as the reference's collection_stats / sym_width give them; the image's md5 where its writer made one"""
    import hashlib
    w = c["cell_bytes"]
    cells = np.frombuffer(bytes.fromhex(c["input_hex"]), dtype=DT[w])
    got, st, values = build_image(lib, cells, w)
    for k in ("n_strings", "min_sym", "max_sym", "n_syms", "max_sym_freq"):
        assert st[k] == c["stats"][k], (c["name"], k, st[k], c["stats"][k])
    assert (st["sb"], st["fb"]) == (c["sb"], c["fb"]), c["name"]
    assert got[:16] == int(c["sb"]).to_bytes(8, "little") + int(c["fb"]).to_bytes(8, "little")
    assert got == oracle_on_ranks(cells, w), c["name"]
    if "runs" in c and c["runs"] is not None and "writer_md5" in c:
        assert (len(got) - 16) // (c["sb"] + c["fb"]) == c["runs"]
    if "writer_md5" in c:
        assert hashlib.md5(got).hexdigest() == c["writer_md5"] and len(got) == c["writer_size"], c["name"]
