"""CPU: collections whose symbols are 2^30 and larger, through the engine logic over the serial test stand-in of the device
primitives (tests/hostsim) -- the general regime of the alphabet compaction, the image packed from the values, the inverter on
64-bit symbols.  The HIP kernels of the compaction are covered by tests/test_wide_alphabet_gpu.py."""
import numpy as np
import pytest

from grlbwt_amd import engine
from oracle import oracle
from tests import bcr_check as bc
from tests import parity
from tests import wide_check as wc


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    oracle.build()
    return simlib.sim_library()


@pytest.mark.parametrize("case", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_final_bytes_equal_oracle_on_ranks(sim, case):
    name, w, n_strings, max_len, n_distinct, lo, hi = case
    for seed in range(4):
        rng = np.random.default_rng([20260007, seed, w, n_distinct])
        cells = wc.collection(rng, w, n_strings, max_len, n_distinct, lo, hi)
        wc.check_final(sim, cells, w, engine.FLAG_FORCE_IDX64 if seed == 3 else 0)


@pytest.mark.parametrize("case", wc.SMALL, ids=[c[0] for c in wc.SMALL])
def test_small_collections_equal_the_textbook_definition(sim, case):
    name, w, n_strings, max_len, n_distinct, lo, hi = case
    for seed in range(3):
        rng = np.random.default_rng([20260008, seed, w])
        cells = wc.collection(rng, w, n_strings, max_len, n_distinct, lo, hi)
        got = wc.check_final(sim, cells, w)
        assert got == bc.naive_rl_bwt(cells.tobytes(), w)


@pytest.mark.parametrize("case", [wc.CASES[1], wc.CASES[4], wc.CASES[6]], ids=lambda c: c[0])
def test_every_stage_is_the_oracles_on_the_rank_text(sim, case):
    """parity.check_stagewise for a compacted build: level 0 is in rank space, so every stage (round counters, parses, grammar,
    pre-BWT, every level's BWT) equals the oracle's trace on the rank text; statistics and image speak of the values."""
    name, w, n_strings, max_len, n_distinct, lo, hi = case
    cells = wc.collection(np.random.default_rng([20260009, w]), w, n_strings, max_len, n_distinct, lo, hi)
    u, inv = wc.ranks_of(cells)
    o = oracle.OracleResult(inv.tobytes(), 8, trace=True)
    with engine.Context(0, engine.FLAG_KEEP_LEVELS, sim) as ctx:
        ctx.upload(cells.tobytes(), w)
        st = ctx.stats()
        for k in ("n_strings", "n_syms", "max_sym_freq", "fb"):
            assert st[k] == o.stats[k], (k, st[k], o.stats[k])
        assert (st["min_sym"], st["max_sym"]) == (int(u[0]), int(u[-1]))
        assert (st["sb"], st["fb"]) == bc.header_widths(cells, w)
        assert ctx.alphabet_size() == len(u) and np.array_equal(ctx.alphabet_download(), u)
        r = 0
        while True:
            info, done = ctx.parse_round()
            oc = o.counters(r)
            assert (info["n_in"], info["n_phrases"], info["dict_syms"], info["n_metasyms"], info["parse_size"], info["sigma"]) == \
                   (oc["n_in"], oc["D"], oc["S"], oc["M"], oc["parse_size"], oc["sigma"]), (r, info, oc)
            sym, rep = o.level_text(r + 1)
            assert np.array_equal(ctx.level_text(r + 1), (sym << np.uint64(1)) | rep.astype(np.uint64)), "parse of level %d differs" % (r + 1)
            r += 1
            if done:
                break
        assert r == o.n_rounds and ctx.round_info(0)["sigma"] == len(u)
        for lvl in range(r):
            g0, g1, hh, ps, pl = ctx.level_grammar(lvl)
            og0, og1, ohh = o.level_grammar(lvl)
            assert np.array_equal(g0, og0) and np.array_equal(g1, og1) and np.array_equal(hh, ohh), "grammar of level %d differs" % lvl
            ops, opl = o.level_prebwt(lvl)
            assert parity._merged(ps, pl) == parity._merged(ops, opl), "pre-BWT of level %d differs" % lvl
        ctx.parse2bwt()
        lvl = r
        while True:
            s, l = ctx.level_bwt(lvl)
            os_, ol = o.level_bwt(lvl)
            assert np.array_equal(s, os_) and np.array_equal(l, ol), "BWT of level %d differs" % lvl
            if lvl == 0:
                break
            lvl, _ = ctx.infer_lvl_bwt()
        assert ctx.result_bytes() == wc.remap_image(o.rl_bwt, u, cells, w)
    o.close()


def test_reference_made_headers_and_images(sim):
    """the reference's collection_stats / sym_width (and its writer where it takes the symbols) on wide collections"""
    wc.check_reference_case(sim, wc.ref_stats_edge())
    cases = wc.golden_cases()
    assert len(cases) >= 6 and {c["sb"] for c in cases} >= {4, 5, 6, 8}
    for c in cases:
        wc.check_reference_case(sim, c)


@pytest.mark.parametrize("mx", [2 ** 64 - 4, 2 ** 64 - 1])
def test_symbols_above_the_header_bound_are_refused(sim, mx):
    cells = np.array([7, mx, 9, 5, mx, 5], dtype=np.uint64)
    with engine.Context(0, 0, sim) as ctx:
        with pytest.raises(engine.GrlbwtError) as e:
            ctx.upload(cells.tobytes(), 8)
        assert e.value.code == wc.ERANGE
        ctx.upload(np.array([7, 2 ** 64 - 5, 9, 5], dtype=np.uint64).tobytes(), 8)          # the bound itself is taken
        assert ctx.alphabet_size() == 4


@pytest.mark.parametrize("w", [4, 8])
def test_a_separator_that_is_not_the_minimum_is_ill_formed(sim, w):
    cells = np.array([2 ** 31 + 5, 2 ** 31 + 1, 2 ** 31 + 3], dtype=wc.DT[w])
    with engine.Context(0, 0, sim) as ctx:
        with pytest.raises(engine.IllFormedInput):
            ctx.upload(cells.tobytes(), w)


@pytest.mark.parametrize("form", ["positions", "runs"])
def test_inverter_round_trip_of_an_sb8_image(sim, form, monkeypatch):
    monkeypatch.setenv("GRLBWT_INVERT", form)
    cells = wc.collection(np.random.default_rng(20260010), 8, 30, 40, 200, 2 ** 20, 2 ** 64 - 5)
    with engine.Context(0, 0, sim) as ctx:
        ctx.upload(cells.tobytes(), 8)
        ctx.build()
        nb, _ = ctx.result_size()
        assert ctx.stats()["sb"] == 8
        out = np.zeros(cells.size, dtype=np.uint64)
        n = ctx.invert_image(ctx.result_device_ptr(), nb, 8, out.ctypes.data, out.size)      # stand-in: device == host
        assert n == cells.size and np.array_equal(out, cells)
        for narrow, dt in ((4, np.uint32), (2, np.uint16), (1, np.uint8)):
            small = np.zeros(cells.size, dtype=dt)
            with pytest.raises(engine.GrlbwtError) as e:
                ctx.invert_image(ctx.result_device_ptr(), nb, narrow, small.ctypes.data, small.size)
            assert e.value.code == wc.EINVAL
        tails = np.zeros(31 * 3, dtype=np.uint64)
        k, _ = ctx.invert_image_tails(ctx.result_device_ptr(), nb, 8, 3, tails.ctypes.data, tails.size)
        ends = np.flatnonzero(cells == cells[-1])
        assert k == len(ends) and all(tails[3 * i + 2] == cells[-1] for i in range(k))
        assert all(tails[3 * i + 1] == cells[e - 1] for i, e in enumerate(ends) if e > 0 and cells[e - 1] != cells[-1])


def test_u32_image_with_five_byte_symbols_round_trips(sim):
    cells = wc.collection(np.random.default_rng(20260011), 4, 20, 30, 50, 2 ** 32 - 500, 2 ** 32 - 1)
    with engine.Context(0, 0, sim) as ctx:
        ctx.upload(cells.tobytes(), 4)
        ctx.build()
        nb, _ = ctx.result_size()
        assert ctx.stats()["sb"] == 5
        out = np.zeros(cells.size, dtype=np.uint32)
        assert ctx.invert_image(ctx.result_device_ptr(), nb, 4, out.ctypes.data, out.size) == cells.size
        assert np.array_equal(out, cells)


def test_split_runs_refuses_symbols_it_cannot_carry(sim):
    """grlbwt_image_split_runs carries symbols in 32 bits: an image with a symbol of 2^32 or more is refused, not cut; one whose
    five-byte symbols all fit 32 bits is re-encoded with its symbols intact"""
    wide = wc.collection(np.random.default_rng(20260012), 8, 10, 20, 20, 2 ** 32 - 10, 2 ** 33)
    fits = wc.collection(np.random.default_rng(20260013), 4, 10, 20, 20, 2 ** 32 - 40, 2 ** 32 - 1)
    for cells, w, ok in ((wide, 8, False), (fits, 4, True)):
        with engine.Context(0, 0, sim) as ctx:
            ctx.upload(cells.tobytes(), w)
            ctx.build()
            nb, nr = ctx.result_size()
            blob = ctx.result_bytes()
            out = np.zeros(16 + 4 * nr * 16 + 64, dtype=np.uint8)
            if not ok:
                with pytest.raises(engine.GrlbwtError) as e:
                    ctx.image_split_runs(ctx.result_device_ptr(), nb, 2, 0, out.ctypes.data, out.size)
                assert e.value.code == wc.EINVAL
                continue
            si = ctx.image_split_runs(ctx.result_device_ptr(), nb, 2, 0, out.ctypes.data, out.size)
            _, _, s0, l0 = bc.parse_rl_bwt(blob)
            _, _, s1, l1 = bc.parse_rl_bwt(out[:si["out_bytes"]].tobytes())
            assert int(l1.max()) <= 3 and np.array_equal(np.repeat(s1, l1.astype(np.int64)), np.repeat(s0, l0.astype(np.int64)))


def test_narrow_collections_take_the_path_they_took(sim):
    """symbols below 2^30 - 8: no compaction, the image is the oracle's on the values themselves"""
    rng = np.random.default_rng(20260014)
    for kind in ("u32", "u64", "u16"):
        data, w = parity.rand_collection(rng, kind)
        with engine.Context(0, 0, sim) as ctx:
            ctx.upload(data, w)
            assert ctx.alphabet_size() == 0
            ctx.build()
            assert ctx.result_bytes() == oracle.rl_bwt(data, w)
    cells = np.array([9, 2 ** 30 - 9, 4, 2, 4, 2], dtype=np.uint32)                  # the largest symbol that is not compacted
    with engine.Context(0, 0, sim) as ctx:
        ctx.upload(cells.tobytes(), 4)
        assert ctx.alphabet_size() == 0


@pytest.mark.parametrize("mine_wide", [False, True])
def test_collection_level_mode_refuses_wide_symbols_on_every_rank(sim, mine_wide):
    """grlbwt_dist_build takes the decision from the GATHERED maximum, right after the statistics' all-gather: a shard of small
    symbols beside a shard of wide ones refuses like the wide one does, and no rank goes on to a second collective.  (Two ranks
    played by one process: the all-gather callback answers with this shard's block and a copy of it that carries the other
    shard's maximum.)"""
    import ctypes as C
    from grlbwt_amd import dist as gd
    small = np.array([9, 100, 4, 2, 4, 2], dtype=np.uint64)
    wide = np.array([9, 2 ** 40, 4, 2, 4, 2], dtype=np.uint64)
    mine, other_max = (wide, 100) if mine_wide else (small, 2 ** 40)
    calls = {"ag": 0, "a2a": 0}

    def ag(user, send, recv, nbytes):
        calls["ag"] += 1
        block = np.frombuffer((C.c_uint8 * nbytes).from_address(send), dtype=np.uint64).copy()
        other = block.copy()
        other[3] = other_max                                  # (n_syms, n_strings, min_sym, max_sym, ...)
        both = np.concatenate([block, other])
        C.memmove(recv, both.ctypes.data, 2 * nbytes)
        return 0

    def a2a(*args):
        calls["a2a"] += 1
        return 1

    comm = gd.CommStruct(0, 2, None, gd._AG(ag), gd._A2A(a2a), 0)
    with engine.Context(0, 0, sim) as ctx:
        ctx.upload(mine.tobytes(), 8)
        assert (ctx.alphabet_size() != 0) == mine_wide
        ctx.L.grlbwt_dist_build.argtypes = [C.c_void_p, C.POINTER(gd.CommStruct)]
        rc = ctx.L.grlbwt_dist_build(ctx._h, C.byref(comm))
        assert rc == wc.ERANGE
        assert b"single-GPU" in ctx.L.grlbwt_last_error(ctx._h)
    assert calls == {"ag": 1, "a2a": 0}
