"""GPU (-m gpu): level 0's pass C writes the .rl_bwt records itself (GRLBWT_ASM_IMAGE, default on) -- against the oracle, against
the emit + pack path (GRLBWT_ASM_IMAGE=0) byte for byte, and with the launch sites checked: a fused build launches the record
sites and no pack_rl_bwt, a collection whose records are wider than 8 bytes still packs.  Pass C takes count + emit at every
level here (GRLBWT_ASM_TWO_PASS=1): the record form replaces that form's emit pass."""
import os

import numpy as np
import pytest

from grlbwt_amd import engine, workloads
from tests import parity, wide_check
from tests.test_engine_logic_sim import _long_run_collection

pytestmark = pytest.mark.gpu

RECORD_SITES = ("asm.emit_rec", "asm.seam")


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__ as g
    lib = g.build_hip()
    assert os.path.exists(lib)
    return lib


def _fuzz(kind, seeds):
    out = []
    for seed in seeds:
        data, w = parity.rand_collection(np.random.default_rng([20260011, seed]), kind)
        out.append((data, w, engine.FLAG_FORCE_IDX64 if seed % 2 else 0))
    return out


# name -> [(bytes, cell width, flags)]
INPUTS = {
    "reads": lambda: [(workloads.sampled_reads(20000, 100, 100000, seed=11).tobytes(), 1, 0)],
    "tokens_idx64": lambda: [(workloads.zipf_tokens(200000, doc_len=500, vocab=20000).tobytes(), 2, engine.FLAG_FORCE_IDX64)],
    "repetitive": lambda: [(workloads.repetitive_copies(40, 50000, seed=3).tobytes(), 1, 0)],
    "long_runs": lambda: [(_long_run_collection(2000, 4, 5), 1, 0)],
    "dups": lambda: _fuzz("dups", range(6)),
    "homopolymer": lambda: _fuzz("homopolymer", range(6)),
}


def _sites(prof):
    """launches per launch site (the level tags folded)"""
    sites = {}
    for name, rec in prof.items():
        site = name.split("#")[0]
        sites[site] = sites.get(site, 0) + int(rec[0])
    return sites


def _profiled_build(lib, data, w, flags):
    with engine.Context(0, flags, lib) as ctx:
        ctx.profile_enable(True)
        ctx.upload(data, w)
        ctx.build()
        return ctx.result_bytes(), _sites(ctx.profile())


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_records_from_pass_c(hip, oracle_mod, monkeypatch, name):
    monkeypatch.setenv("GRLBWT_ASM_TWO_PASS", "1")
    entered = 0
    cases = INPUTS[name]()
    for data, w, flags in cases:
        monkeypatch.delenv("GRLBWT_ASM_IMAGE", raising=False)
        fused = parity.check_final(hip, data, w, flags)
        again, sites = _profiled_build(hip, data, w, flags)
        assert again == fused
        if len(cases) == 1 or sites.get("asm.count", 0):        # (a fuzz collection of one round has no pass C at all)
            assert sites.get("pack_rl_bwt", 0) == 0, sorted(sites)
            for s in RECORD_SITES:                  # a path that was never entered must not pass silently
                assert sites.get(s, 0) >= 1, (s, sorted(k for k in sites if k.startswith("asm.")))
            entered += 1
        else:
            assert sites.get("pack_rl_bwt", 0) >= 1, sorted(sites)
        monkeypatch.setenv("GRLBWT_ASM_IMAGE", "0")
        packed, sites = _profiled_build(hip, data, w, flags)
        assert packed == fused, "the image differs from emit + pack's (%d vs %d bytes)" % (len(fused), len(packed))
        assert sites.get("pack_rl_bwt", 0) >= 1 and sites.get("asm.emit_rec", 0) == 0, sorted(sites)
    assert entered * 2 > len(cases), "%d of %d builds went through pass C" % (entered, len(cases))


def test_records_wider_than_8_bytes_still_pack(hip, monkeypatch):
    monkeypatch.setenv("GRLBWT_ASM_TWO_PASS", "1")
    cells = workloads.wide_tokens(200000, 500, 20000, 64)
    got = wide_check.check_final(hip, cells, 8)
    again, sites = _profiled_build(hip, cells.tobytes(), 8, 0)
    assert again == got
    assert sites.get("pack_rl_bwt", 0) >= 1 and sites.get("asm.emit_rec", 0) == 0, sorted(sites)
