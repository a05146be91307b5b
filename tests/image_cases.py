"""Shared by tests/test_image_consumers.py and tests/golden/make_image_fixtures.py: .rl_bwt images the engine did NOT make.

The recipe is code (numpy, seeded), the expected outputs are data (tests/golden/ref_image_consumers.json holds md5/size of the
image each recipe gives and of what the reference's programs made of it).  An image built by the engine is always friendly:
maximal runs, no empty record, sb of 1 or 2, the narrowest fb, a total far below 2^32.  The images here are the other kind,
at the sizes the consumer kernels change path at: 64-bit bitmap words, 16 run starts per lane (BuildBitsFn), one lane per
piece (SplitRunsFn), the 32/64-bit index dispatch at 2^32 - 256 symbols.

    make_image(sb, fb, syms, lens) -> bytes        the container: two uint64 widths, then (sym: sb bytes LE, len: fb bytes LE)
    decode(syms, lens) -> uint64[n]                by definition: np.repeat, an empty record contributes nothing
    CASES                                          the named list; .giant images are never expanded
"""
import zlib

import numpy as np

WIDTHS = [(1, 1), (1, 2), (1, 3), (2, 3), (3, 5), (4, 4), (5, 8), (8, 8)]
IDX32_LIMIT = 2 ** 32 - 256          # totals of this size or more take the 64-bit index instantiation of a consumer
EINVAL = -22


def make_image(sb, fb, syms, lens):
    syms = np.asarray(syms, dtype=np.uint64).reshape(-1)
    lens = np.asarray(lens, dtype=np.uint64).reshape(-1)
    assert syms.shape == lens.shape and 1 <= sb <= 8 and 1 <= fb <= 8
    assert sb == 8 or not len(syms) or int(syms.max()) < 1 << (8 * sb)
    assert fb == 8 or not len(lens) or int(lens.max()) < 1 << (8 * fb)
    rec = np.zeros((len(syms), sb + fb), dtype=np.uint8)
    for b in range(sb):
        rec[:, b] = ((syms >> np.uint64(8 * b)) & np.uint64(255)).astype(np.uint8)
    for b in range(fb):
        rec[:, sb + b] = ((lens >> np.uint64(8 * b)) & np.uint64(255)).astype(np.uint8)
    return int(sb).to_bytes(8, "little") + int(fb).to_bytes(8, "little") + rec.tobytes()


def decode(syms, lens):
    return np.repeat(np.asarray(syms, dtype=np.uint64), np.asarray(lens, dtype=np.uint64).astype(np.int64))


def canonical(syms, lens):
    """The decoded string as maximal runs, without expanding it: empty records dropped, equal neighbours merged."""
    syms = np.asarray(syms, dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.uint64)
    keep = lens != 0
    syms, lens = syms[keep], lens[keep]
    if not len(syms):
        return syms, lens
    head = np.concatenate([[True], syms[1:] != syms[:-1]])
    return syms[head], np.add.reduceat(lens, np.flatnonzero(head))


class Case:
    def __init__(self, name, sb, fb, syms, lens, splits=(), giant=False):
        self.name, self.sb, self.fb = name, sb, fb
        self.syms = np.asarray(syms, dtype=np.uint64).reshape(-1)
        self.lens = np.asarray(lens, dtype=np.uint64).reshape(-1)
        self.splits = [(int(a), int(b)) for a, b in splits]
        self.giant = giant
        self.R = len(self.syms)
        self.n = int(self.lens.sum(dtype=np.uint64)) if self.R else 0
        self.splittable = not self.R or int(self.syms.max()) < 2 ** 32      # split_runs refuses wider symbols

    def image(self):
        return make_image(self.sb, self.fb, self.syms, self.lens)


def pool(sb):
    """Run symbols of a width: 0 is always there (null_char), and from sb = 2 on values above 255 whose low byte is 0, 255, ..."""
    p = [0, 10, 65, 67, 255]
    if sb >= 2:
        p += [256, 0x1FF, 0x4100, (1 << 16) - 1]
    if sb >= 3:
        p += [1 << 16, (1 << 24) - 1]
    if sb >= 4:
        p += [1 << 30, (1 << 31) + 5, (1 << 32) - 1]
    return np.array(p, dtype=np.uint64)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()) + 20261018)


def _draw_splits(rng, n, k):
    """k (bits, block) settings for a small image of n symbols: every bits value, blocks around and far from n.  (Blocks of 1 and
    2 are set by hand in a few cases: the reference's program counts the records of a block in a vector of block_size entries
    and trips its own assertion wherever a block holds that many.)"""
    bits = [1, 2, 3, 8, 9, 16]
    blocks = [7, 64, 64, n + 5, max(n, 1), 0]
    out = []
    while len(out) < k:
        s = (bits[int(rng.integers(len(bits)))], blocks[int(rng.integers(len(blocks)))])
        if s[0] == 1 and s[1]:                # (L = 1: a block holds block_size records; "split:multiples" has that)
            s = (3, s[1])
        if s == (2, 7):                       # (L = 3 and empty records: seven records in a block of 7 here and there)
            s = (8, 7)
        if s not in out:
            out.append(s)
    return out


def _syms(rng, sb, R, repeat=0.0):
    p = pool(sb)
    s = p[rng.integers(0, len(p), size=R)]
    for i in range(1, R):                      # maximal unless asked otherwise
        if rng.random() < repeat:
            s[i] = s[i - 1]
        elif s[i] == s[i - 1]:
            s[i] = p[(int(np.flatnonzero(p == s[i])[0]) + 1) % len(p)]
    return s


def _build():
    cases = []

    def add(name, sb, fb, syms, lens, splits=None, k=3, giant=False):
        c = Case(name, sb, fb, syms, lens, giant=giant)
        if splits is None:
            splits = _draw_splits(_rng("splits:" + name), c.n, k) if c.splittable else []
            if sb == 8:                       # (the reference's writer refuses every symbol of an 8-byte field: one setting, by definition)
                splits = splits[:1]
        c.splits = [(int(a), int(b)) for a, b in splits]
        cases.append(c)

    # ---- run counts: 0 (a 16-byte image), below 10 (decile clamp), around the 16 run starts a BuildBitsFn lane takes
    for R in (0, 1, 2, 9, 10, 15, 16, 17, 33):
        rng = _rng("runs:%d" % R)
        add("runs:R=%d" % R, 1, 2, _syms(rng, 1, R), rng.integers(1, 300, size=R), splits=None if R else [(8, 64), (3, 0)])
    for sb, fb in WIDTHS:
        if (sb, fb) != (1, 2):
            add("runs:R=0,sb=%d,fb=%d" % (sb, fb), sb, fb, [], [], splits=[(8, 0)])

    # ---- run ends on and around the 64-bit words of the run-start bitmap, and a run over several whole words
    ends_lens = [63, 1, 1, 62, 1, 64 * 3 + 5, 30, 64 * 4 - 35, 1]          # ends at 63 64 65 127 128 325 355 576 577
    for sb, fb in ((1, 2), (2, 3)):
        rng = _rng("ends:%d" % sb)
        add("ends:sb=%d,fb=%d" % (sb, fb), sb, fb, _syms(rng, sb, len(ends_lens)), ends_lens, splits=[(3, 64), (8, 7), (9, 64), (2, 65), (16, 0)])

    # ---- empty records: first, last, two and three in a row, on a word boundary (64, 128); and nothing but empty records
    empty_lens = [0, 5, 0, 0, 59, 0, 7, 0, 0, 0, 57, 0, 3, 9, 61, 0, 0, 2, 0]      # the boundaries 64 and 128 each carry empty records
    for sb, fb in WIDTHS:
        rng = _rng("empty:%d,%d" % (sb, fb))
        add("empty:sb=%d,fb=%d" % (sb, fb), sb, fb, _syms(rng, sb, len(empty_lens), repeat=0.3), empty_lens,
            splits=[(3, 64), (16, 7), (8, 2)] if (sb, fb) == (1, 1) else None, k=3)
        add("allempty:sb=%d,fb=%d" % (sb, fb), sb, fb, _syms(rng, sb, 5, repeat=0.3), [0] * 5, splits=[(4, 64)] if sb == 4 else [(4, 0)])

    # ---- non-maximal runs: equal neighbours, with and without empty records between them
    for sb, fb in ((1, 1), (2, 3), (4, 4)):
        p = pool(sb)
        A, B, Cc, Z = p[-1], p[2], p[3], p[0]
        syms = [A, A, B, B, B, Cc, A, Cc, Cc, Cc, Cc, Z, Z, Z, B, A, A]
        lens = [3, 4, 60, 0, 5, 1, 0, 2, 0, 0, 9, 7, 0, 7, 1, 200, 55]
        add("nonmax:sb=%d,fb=%d" % (sb, fb), sb, fb, syms, lens, splits=[(3, 1), (2, 64), (8, 64)] if sb == 1 else None)

    # ---- every header width on a few hundred seeded records: empty ones, repeated symbols, a few long runs
    for sb, fb in WIDTHS:
        rng = _rng("random:%d,%d" % (sb, fb))
        R = int(rng.integers(200, 400))
        lens = rng.integers(0, 40, size=R)
        lens[rng.random(R) < 0.1] = 0
        cap = min((1 << (8 * fb)) - 1, 5000)
        big = rng.integers(0, R, size=6)
        lens[big] = rng.integers(cap // 2, cap + 1, size=6)
        add("random:sb=%d,fb=%d" % (sb, fb), sb, fb, _syms(rng, sb, R, repeat=0.3), lens, k=3)
    rng = _rng("random:many")
    R = 3000
    lens = rng.integers(0, 50, size=R)
    lens[rng.random(R) < 0.15] = 0
    add("random:R=3000,sb=2,fb=1", 2, 1, _syms(rng, 2, R, repeat=0.2), lens, k=3)

    # ---- split_runs: lengths that are multiples of L = 2^bits - 1 (3, 7, 255) and of the block (7, 64), runs that end on a
    # block boundary, L below and above the block -- every (bits, block) of the issue's lists
    mult = [7, 14, 21, 64, 128, 3, 6, 9, 49, 1, 0, 63, 2, 255, 510, 43, 0, 64]
    rng = _rng("split:multiples")
    c = Case("split:multiples", 1, 2, _syms(rng, 1, len(mult), repeat=0.2), mult)
    c.splits = [(b, k) for b in (1, 2, 3, 8, 9, 16) for k in (7, 64, c.n + 5, c.n, 0) if (b, k) != (1, 7)] + [(1, 1), (2, 2), (8, 1)]
    cases.append(c)

    # ---- a symbol of 2^32 and more: plain and rle take its low byte (2^32 is not the null character), split_runs refuses it
    add("sym:2^32,sb=8,fb=8", 8, 8, [0, 1 << 32, 65, (1 << 40) + 7, 1 << 32, (1 << 63) + 256, 0, (1 << 32) + 67], [3, 70, 0, 5, 64, 2, 9, 1])
    add("sym:2^32,sb=5,fb=8", 5, 8, [1 << 32, 0, (1 << 39) + 255, 256], [64, 1, 130, 0])

    # ---- giant lengths, never expanded: the two sides of the 64-bit dispatch, lengths whose uint32 cast is 0 or small
    G = dict(giant=True)
    add("giant:total=2^32-257", 1, 5, [65, 0, 67, 65, 255], [1 << 31, (1 << 31) - 257 - 7, 0, 7, 0], splits=[(33, 0), (33, 1 << 31)], **G)
    add("giant:total=2^32-256", 1, 5, [65, 0, 67, 65, 255], [1 << 31, (1 << 31) - 256 - 7, 0, 7, 0], splits=[(40, 1 << 31), (63, 0)], **G)
    add("giant:total=2^41", 1, 8, [65, 67, 67, 0, 10, 65, 255, 0, 65, 67, 10, 0],
        [1 << 32, (1 << 32) + 1, 1 << 40, 3, (1 << 32) - 1, 0, (1 << 40) + 12345, 1, 70000, 255, 256, 65535],
        splits=[(33, 1 << 38), (63, 1 << 38), (40, 0)], **G)
    add("giant:sb=2,fb=5", 2, 5, [256, 0x1FF, 0, 0x4100], [(1 << 32) + 5, 1 << 32, 0, (1 << 33) - 1], splits=[(40, 1 << 31), (33, 0)], **G)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- split_runs by definition (for the settings the reference's program aborts on) ---------------------------------------
def check_split_by_definition(case, bits, block, out_blob, info):
    """Same decoded string, no record longer than L, none across a multiple of the block, the header comment's arithmetic."""
    from tests import bcr_check as bc
    L = (1 << bits) - 1
    sb, fb, sym, ln = bc.parse_rl_bwt(out_blob)
    assert (sb, fb) == (case.sb, (bits + 7) // 8)
    a, b = canonical(sym, ln), canonical(case.syms, case.lens)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "split image decodes to another string"
    assert not len(ln) or int(ln.max()) <= L
    if block and len(ln):
        pos = np.concatenate([[0], np.cumsum(ln, dtype=np.uint64)]).astype(np.uint64)
        full = ln != 0
        first, last = pos[:-1][full], pos[1:][full] - np.uint64(1)
        assert np.array_equal(first // np.uint64(block), last // np.uint64(block)), "a record crosses a block boundary"
    pieces = int(sum(1 if l == 0 else -(-int(l) // L) for l in case.lens))
    cuts = (case.n - 1) // block if block and case.n else 0
    assert info["runs_before"] == case.R and info["n_syms"] == case.n
    assert info["overflow_splits"] == pieces - case.R and info["block_splits"] == cuts
    assert info["runs_after"] == pieces + cuts == len(ln)
    assert info["n_blocks"] == ((1 + (case.n - 1) // block) if block and case.n else 0)
    assert info["out_bytes"] == len(out_blob) == 16 + len(ln) * (sb + fb)
