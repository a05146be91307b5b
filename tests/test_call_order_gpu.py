"""GPU (-m gpu): the call-order contract of the stage-wise C API (the table of include/grlbwt_hip.h) on the device, against the
model of tests/call_order_cases.py and the oracle, and the state a context and the process-wide runtime keep between calls:
a caller's stream, the debug flag, refused calls beside a live context, one context over texts of every width.  The full
enumeration of call sequences runs on the stand-in (tests/test_call_order_sim.py); here a list that holds every refused and
every no-op transition."""
import os

import pytest

from grlbwt_amd import engine
from tests import base_case_cases
from tests import call_order_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__ as g
    lib = g.build_hip()
    assert os.path.exists(lib)
    return lib


def reads():
    return base_case_cases.reads()


def tokens():
    return base_case_cases.tokens()


def image_now(ctx):
    """the image cloned on torch's default stream the moment the call before has returned: no synchronisation by the caller"""
    import torch
    from grlbwt_amd import dist as gdist
    nb, _ = ctx.result_size()
    return bytes(gdist._view(ctx.result_device_ptr(), nb, torch.device("cuda:0")).clone().cpu().numpy())


@pytest.mark.parametrize("kind,flags", [("reads", 0), ("reads", engine.FLAG_FORCE_IDX64), ("u16_tokens", engine.FLAG_FORCE_IDX64)],
                         ids=["reads-idx32", "reads-idx64", "u16_tokens-idx64"])
def test_sequences_with_every_refused_and_no_op_transition(hip, oracle_mod, monkeypatch, kind, flags):
    monkeypatch.delenv(cases.RATIO, raising=False)
    data, cell_bytes = (reads(), 1) if kind == "reads" else (tokens(), 2)
    want, rounds = cases.expected(data, cell_bytes)
    assert rounds >= 3, rounds
    cases.assert_covers(cases.DEVICE_SEQUENCES, rounds)
    cases.check_sequences(hip, cases.DEVICE_SEQUENCES, data, cell_bytes, flags, rounds, want)


@pytest.mark.parametrize("asm_image", [None, "0"], ids=["asm_image_default", "asm_image_0"])
@pytest.mark.parametrize("kind", ["reads", "wide_u64"])
def test_done_is_idempotent(hip, oracle_mod, monkeypatch, kind, asm_image):
    """the image's pointer and bytes after a second build, induce_phase and parse_round in DONE: written by level 0's stream
    merge (the default), by the pack pass (GRLBWT_ASM_IMAGE=0), and one lane per run (wide_u64: records of more than 8 bytes)"""
    if asm_image is None:
        monkeypatch.delenv("GRLBWT_ASM_IMAGE", raising=False)
    else:
        monkeypatch.setenv("GRLBWT_ASM_IMAGE", asm_image)
    if kind == "reads":
        cases.check_idempotent_done(hip, reads(), 1, cases.expected(reads())[0])
    else:
        cells, want = cases.wide_expected(8)
        cases.check_idempotent_done(hip, cells.tobytes(), 8, want)


def test_one_context_text_after_text(hip, oracle_mod):
    cases.check_context_reuse(hip, reads(), tokens())


def test_build_on_the_callers_stream_and_back(hip, oracle_mod):
    """grlbwt_ctx_set_stream: the text is produced on a stream of the caller's and that stream synchronised, the build runs on
    it and its image is complete when build() returns; set_stream(0) goes back to the engine's own stream.  The context is
    closed while the stream lives; the next context of the process builds the same image."""
    import torch
    import numpy as np
    want = cases.expected(reads())[0]
    host = torch.from_numpy(np.frombuffer(reads(), dtype=np.uint8).copy())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = host.to("cuda:0").clone()
    side.synchronize()
    ctx = engine.Context(0, 0, hip)
    try:
        ctx.set_stream(side.cuda_stream)
        ctx.attach_device(dev.data_ptr(), dev.numel(), 1, keepalive=dev)
        ctx.build()
        assert image_now(ctx) == want
        ctx.set_stream(0)
        ctx.attach_device(dev.data_ptr(), dev.numel(), 1, keepalive=dev)
        ctx.build()
        assert image_now(ctx) == want
    finally:
        ctx.close()
    del side
    with engine.Context(0, 0, hip) as ctx:
        ctx.attach_device(dev.data_ptr(), dev.numel(), 1, keepalive=dev)
        ctx.build()
        assert image_now(ctx) == want


def test_sync_debug_flag_builds_the_same_image_and_ends_with_its_context(hip, oracle_mod):
    want = cases.expected(reads())[0]
    for flags in (engine.FLAG_SYNC_DEBUG, 0):
        with engine.Context(0, flags, hip) as ctx:
            ctx.upload(reads(), 1)
            ctx.build()
            assert ctx.result_bytes() == want


def test_refused_calls_leave_a_live_context_usable(hip, oracle_mod):
    """a text that is not 16-byte aligned, and a second context on a device that is not there: both refused, and the first
    context builds as before"""
    import torch
    import numpy as np
    want = cases.expected(reads())[0]
    raw = torch.from_numpy(np.frombuffer(reads(), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    with engine.Context(0, 0, hip) as ctx:
        ctx.attach_device(raw.data_ptr(), raw.numel(), 1, keepalive=raw)
        with pytest.raises(engine.GrlbwtError) as e:
            ctx.attach_device(raw.data_ptr() + 1, raw.numel() - 1, 1, keepalive=raw)
        assert e.value.code == cases.EINVAL
        ctx.build()
        assert ctx.result_bytes() == want
        with pytest.raises(engine.GrlbwtError):
            engine.Context(torch.cuda.device_count(), 0, hip)
        ctx.attach_device(raw.data_ptr(), raw.numel(), 1, keepalive=raw)
        ctx.build()
        assert ctx.result_bytes() == want
