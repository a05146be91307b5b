"""GPU: collections whose symbols are 2^30 and larger through the HIP library -- the alphabet compaction kernels in each of
their regimes, the image packed from the values, the device inverter on 64-bit symbols, the command line."""
import os
import subprocess

import numpy as np
import pytest

from grlbwt_amd import engine, workloads
from tests import bcr_check as bc
from tests import wide_check as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__ as g
    lib = g.build_hip()
    assert os.path.exists(lib)
    from oracle import oracle
    oracle.build()
    return lib


def _dev(a):
    """numpy array of any unsigned width -> torch tensor on the device holding the same bytes (16-byte aligned)"""
    import torch
    signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed).copy()).to("cuda:0")


def _host(t, dt):
    return t.cpu().numpy().view(dt)


@pytest.mark.parametrize("case", wc.CASES + wc.SMALL, ids=[c[0] for c in wc.CASES + wc.SMALL])
def test_final_bytes_equal_oracle_on_ranks(hip, case):
    name, w, n_strings, max_len, n_distinct, lo, hi = case
    for seed in range(4):
        rng = np.random.default_rng([20260007, seed, w, n_distinct])
        cells = wc.collection(rng, w, n_strings, max_len, n_distinct, lo, hi)
        got = wc.check_final(hip, cells, w, engine.FLAG_FORCE_IDX64 if seed == 3 else 0)
        if case in wc.SMALL:
            assert got == bc.naive_rl_bwt(cells.tobytes(), w)


def test_reference_made_headers_and_images(hip):
    wc.check_reference_case(hip, wc.ref_stats_edge())
    for c in wc.golden_cases():
        wc.check_reference_case(hip, c)


def _compact(hip, cells, flags=0):
    import torch
    w = cells.dtype.itemsize
    u, inv = wc.ranks_of(cells)
    src = _dev(cells)
    ranks = torch.full((cells.size + 8,), -1, dtype=torch.int32, device="cuda:0")
    values = torch.zeros(len(u) + 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with engine.Context(0, flags, hip) as ctx:
        ctx.profile_enable(True)
        k = ctx.alphabet_compact(src.data_ptr(), cells.size, w, ranks.data_ptr(), values.data_ptr(), len(u))
        prof = ctx.profile()
        assert k == len(u)
        torch.cuda.synchronize()
        assert np.array_equal(_host(values, np.uint64)[:k], u), "sorted values differ from np.unique"
        r = _host(ranks, np.uint32)
        assert np.array_equal(r[:cells.size].astype(np.uint64), inv), "ranks differ from np.unique's inverse"
        assert np.all(r[cells.size:] == 0xFFFFFFFF), "written behind the last cell"
        if len(u) > 1:                                                       # too small an output: refused, the count still reported
            with pytest.raises(engine.GrlbwtError) as e:
                ctx.alphabet_compact(src.data_ptr(), cells.size, w, ranks.data_ptr(), values.data_ptr(), len(u) - 1)
            assert e.value.code == wc.EINVAL
    return set(prof)


def _values(rng, w, sigma, kind="full"):
    hi = 2 ** (8 * w) - 5
    v = set()
    while len(v) < sigma:
        x = rng.integers(0, 2 ** 63, size=2 * (sigma - len(v)) + 8, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=2 * (sigma - len(v)) + 8, dtype=np.uint64)
        if kind == "top":
            x = (x >> np.uint64(32)) << np.uint64(32)                        # values that differ only in the top 32 bits
        elif kind == "bottom":
            x = (x & np.uint64(0xFFFFFFFF)) | np.uint64(0x7A5A5A5A00000000)  # ... only in the bottom 32
        if w == 4:
            x = x >> np.uint64(32)
        v.update(int(y) for y in x.tolist() if int(y) <= hi)
    return np.array(sorted(v)[:sigma], dtype=wc.DT[w])


@pytest.mark.parametrize("w", [4, 8])
@pytest.mark.parametrize("regime,sigma,n", [("lds", 5, 100003), ("lds", 3000, 1 << 20), ("lds", 4096, 300001), ("table", 4097, 300001),
                                            ("table", 100000, (1 << 21) + 7), ("general", 1000000, 1000003)])
def test_compaction_regimes(hip, w, regime, sigma, n):
    """every regime against np.unique; n is not a multiple of a lane's four cells nor of a workgroup's tile"""
    rng = np.random.default_rng([20260015, w, sigma])
    vals = _values(rng, w, sigma)
    cells = vals[rng.integers(0, sigma, size=n)]
    cells[:sigma] = vals                                                     # every value occurs
    names = _compact(hip, cells, engine.FLAG_FORCE_IDX64 if sigma == 3000 else 0)
    want = {"lds": "alpha.rank_lds", "table": "alpha.rank_table", "general": "alpha.sort_pairs"}[regime]
    assert any(k.startswith(want) for k in names), (want, sorted(names))
    assert regime == "general" or not any(k.startswith("alpha.sort_pairs") for k in names)


@pytest.mark.parametrize("w", [4, 8])
def test_general_regime_forced_by_the_switch(hip, w, monkeypatch):
    monkeypatch.setenv("GRLBWT_ALPHA_TABLE_BITS", "2")
    rng = np.random.default_rng([20260016, w])
    vals = _values(rng, w, 40)
    cells = vals[rng.integers(0, 40, size=5001)]
    names = _compact(hip, cells)
    assert any(k.startswith("alpha.sort_pairs") for k in names), sorted(names)
    monkeypatch.delenv("GRLBWT_ALPHA_TABLE_BITS")
    col = wc.collection(rng, w, 30, 40, 300, 2 ** 31, 2 ** (8 * w) - 5)
    monkeypatch.setenv("GRLBWT_ALPHA_TABLE_BITS", "2")
    wc.check_final(hip, col, w)


@pytest.mark.parametrize("w", [4, 8])
def test_compaction_edges(hip, w):
    _compact(hip, np.full(70001, 2 ** 31 + 3, dtype=wc.DT[w]))               # all cells equal
    _compact(hip, np.array([2 ** 31 + 3], dtype=wc.DT[w]))                    # one cell
    rng = np.random.default_rng([20260017, w])
    if w == 8:
        for kind in ("top", "bottom"):
            vals = _values(rng, 8, 20000, kind)
            _compact(hip, vals[rng.integers(0, len(vals), size=200003)])
    # an unaligned cell buffer takes the scalar loads
    import torch
    vals = _values(rng, w, 500)
    cells = vals[rng.integers(0, 500, size=40001)]
    u, inv = wc.ranks_of(cells)
    buf = _dev(np.concatenate([np.zeros(1, dtype=wc.DT[w]), cells]))
    ranks = torch.zeros(cells.size, dtype=torch.int32, device="cuda:0")
    values = torch.zeros(len(u), dtype=torch.int64, device="cuda:0")
    with engine.Context(0, 0, hip) as ctx:
        assert ctx.alphabet_compact(buf.data_ptr() + w, cells.size, w, ranks.data_ptr(), values.data_ptr(), len(u)) == len(u)
    assert np.array_equal(_host(ranks, np.uint32).astype(np.uint64), inv) and np.array_equal(_host(values, np.uint64), u)


def test_wide_tokens_32M_build_and_invert(hip, monkeypatch):
    """workloads.wide_tokens, -a 8, 64-bit values: the image equals the image of the same collection given as its np.unique
    ranks with -a 4 (the oracle-pinned path) with the symbols mapped back and the wide header; both forms of the inversion
    return the input cells."""
    import torch
    cells = workloads.wide_tokens(32 * 1000 * 1001, 1000, 65000, 64)
    u, inv = wc.ranks_of(cells)
    assert int(u[-1]) >= 2 ** 63 and len(u) > 30000
    dev = _dev(cells)
    rdev = _dev(inv.astype(np.uint32))
    torch.cuda.synchronize()
    with engine.Context(0, 0, hip) as ctx:
        ctx.attach_device(rdev.data_ptr(), rdev.numel(), 4, keepalive=rdev)
        assert ctx.alphabet_size() == 0
        ctx.build()
        rank_blob = ctx.result_bytes()
    del rdev
    want = wc.remap_image(rank_blob, u, cells, 8)
    with engine.Context(0, 0, hip) as ctx:
        ctx.attach_device(dev.data_ptr(), dev.numel(), 8, keepalive=dev)
        assert ctx.alphabet_size() == len(u) and np.array_equal(ctx.alphabet_download(), u)
        ctx.build()
        st = ctx.stats()
        assert (st["sb"], st["min_sym"], st["max_sym"]) == (8, int(u[0]), int(u[-1]))
        got = ctx.result_bytes()
        assert got == want
        nb, _ = ctx.result_size()
        for form in ("positions", "runs"):
            monkeypatch.setenv("GRLBWT_INVERT", form)
            back = torch.zeros_like(dev)
            torch.cuda.synchronize()
            n = ctx.invert_image(ctx.result_device_ptr(), nb, 8, back.data_ptr(), back.numel())
            torch.cuda.synchronize()
            assert n == dev.numel() and torch.equal(back, dev), form
            del back
        small = torch.zeros(dev.numel(), dtype=torch.int32, device="cuda:0")
        with pytest.raises(engine.GrlbwtError) as e:
            ctx.invert_image(ctx.result_device_ptr(), nb, 4, small.data_ptr(), small.numel())
        assert e.value.code == wc.EINVAL


def test_cli_file_to_file(hip, tmp_path):
    import __graft_entry__ as g
    cli = g.build_cli()
    cells = wc.collection(np.random.default_rng(20260018), 8, 200, 50, 3000, 2 ** 33, 2 ** 64 - 5)
    src = tmp_path / "wide.u64"
    src.write_bytes(cells.tobytes())
    p = subprocess.run([cli, str(src), "-a", "8", "-o", str(tmp_path / "wide")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert open(tmp_path / "wide.rl_bwt", "rb").read() == wc.oracle_on_ranks(cells, 8)
