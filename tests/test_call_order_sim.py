"""CPU: the call-order contract of the stage-wise C API (the table of include/grlbwt_hip.h) over the serial stand-in of the device
primitives, against the model of tests/call_order_cases.py and the oracle.  The stand-in runs the same orchestration and the
same C layer as the device library; tests/test_call_order_gpu.py runs a chosen part of this on the device."""
import pytest

from grlbwt_amd import engine
from tests import call_order_cases as cases
from tests import parity


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


def test_the_model_counts_what_the_table_says():
    assert len(cases.all_sequences()) == 258
    idle = cases.idle_transitions(5)
    assert len(idle) == 18 and sorted(idle.values()).count("refused") == 10
    cases.assert_covers(cases.all_sequences(), 5)
    cases.assert_covers(cases.DEVICE_SEQUENCES, 5)


CONFIGS = {
    "flags0": (cases.small_reads, 1, 0, None),
    "idx64_u16": (cases.small_tokens, 2, engine.FLAG_FORCE_IDX64, None),
    "ratio0": (cases.small_reads, 1, 0, "0"),
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_sequence_of_up_to_three_calls(sim, oracle_mod, monkeypatch, config):
    """each call's code is the model's, result_size succeeds exactly in DONE, and a build afterwards gives the oracle's image"""
    data_fn, cell_bytes, flags, ratio = CONFIGS[config]
    if ratio is None:
        monkeypatch.delenv(cases.RATIO, raising=False)
    else:
        monkeypatch.setenv(cases.RATIO, ratio)
    data = data_fn()
    want, rounds = cases.expected(data, cell_bytes)
    # (the reads take four rounds or more; Zipf tokens take three whatever their size, which still leaves a PARTLY PARSED state
    # of two depths and an induction of three levels)
    assert rounds >= (4 if cell_bytes == 1 else 3), rounds
    if config == "flags0":      # a plain build of these reads stops parsing early: build() from LOADED is the base case's path
        assert cases.rounds_of_plain_build(sim, data, cell_bytes, flags) < rounds
    if config == "ratio0":
        assert cases.rounds_of_plain_build(sim, data, cell_bytes, flags) == rounds
    cases.check_sequences(sim, cases.all_sequences(), data, cell_bytes, flags, rounds, want)


@pytest.mark.parametrize("data", [b"\n\n\n", b"A\n"], ids=["empty_strings", "one_string"])
def test_every_sequence_on_a_text_of_one_level(sim, oracle_mod, monkeypatch, data):
    monkeypatch.delenv(cases.RATIO, raising=False)
    want, rounds = cases.expected(data, 1)
    assert rounds == 1
    cases.check_sequences(sim, cases.all_sequences(), data, 1, 0, rounds, want)


@pytest.mark.parametrize("kind", ["reads", "u16_tokens"])
def test_stagewise_parity_with_idle_calls_between_the_steps(sim, oracle_mod, kind):
    """parity.check_stagewise, every level's parse, grammar, pre-BWT and BWT against the oracle's, while every call the table
    refuses or makes a no-op is fired between its steps"""
    data, cell_bytes = (cases.small_reads(), 1) if kind == "reads" else (cases.small_tokens(), 2)
    rounds = cases.expected(data, cell_bytes)[1]
    hook = cases.IdleCalls(rounds)
    parity.check_stagewise(sim, data, cell_bytes, engine.FLAG_KEEP_LEVELS, between=hook)
    assert set(hook.fired) == set(cases.idle_transitions(rounds)), sorted(set(cases.idle_transitions(rounds)) - set(hook.fired))


@pytest.mark.parametrize("asm_image", [None, "0"], ids=["asm_image_default", "asm_image_0"])
@pytest.mark.parametrize("kind", ["reads", "wide_u64"])
def test_done_is_idempotent(sim, oracle_mod, monkeypatch, kind, asm_image):
    """a second build, induce_phase and parse_round in DONE leave the image's pointer and bytes alone.  wide_u64: records of more
    than 8 bytes, packed one lane per run"""
    if asm_image is None:
        monkeypatch.delenv("GRLBWT_ASM_IMAGE", raising=False)
    else:
        monkeypatch.setenv("GRLBWT_ASM_IMAGE", asm_image)
    if kind == "reads":
        cases.check_idempotent_done(sim, cases.small_reads(), 1, cases.expected(cases.small_reads())[0])
    else:
        cells, want = cases.wide_expected(8)
        cases.check_idempotent_done(sim, cells.tobytes(), 8, want)


def test_one_context_text_after_text(sim, oracle_mod):
    """cell widths 1, 2 and 8 (compacted), a refused load in between, then the first text again: nothing of a text outlives it"""
    cases.check_context_reuse(sim, cases.small_reads(), cases.small_tokens())


def test_build_refused_for_a_changed_borrowed_text_works_once_the_bytes_are_back(sim, oracle_mod):
    """the refusal of test_borrowed_text_that_changes_after_attach_is_refused (tests/test_gpu_parity.py), the stand-in's host
    buffer standing for device memory: the build is refused, the bytes are put back, the same build gives the oracle's image"""
    good = cases.borrowed_reads()
    buf = cases.aligned_copy(good)
    with engine.Context(0, 0, sim) as ctx:
        ctx.attach_device(buf.ctypes.data, buf.size, 1, keepalive=buf)
        odd = buf[1::2]
        odd[odd == ord("A")] = ord("R")          # a value the statistics did not see
        with pytest.raises(engine.GrlbwtError, match="has changed since its statistics") as e:
            ctx.build()
        assert e.value.code == cases.EINVAL and cases.result_size_code(ctx) == cases.EINVAL
        buf[:] = good
        ctx.build()
        assert ctx.result_bytes() == cases.expected(good.tobytes())[0]


def test_a_refusal_before_any_engine_work_brings_its_own_message(sim, oracle_mod):
    """grlbwt_last_error after an EINVAL that never reached the engine names that refusal, not the failure before it"""
    with engine.Context(0, 0, sim) as ctx:
        with pytest.raises(engine.IllFormedInput):
            ctx.upload(cases.ILL_FORMED, 1)
        cases.check_no_text(ctx, "ill formed")
        ctx.upload(b"ACGT\nAC\n", 1)
        with pytest.raises(engine.GrlbwtError) as e:
            ctx.result_size()
        assert e.value.code == cases.EINVAL and "no image yet" in str(e.value)
        with pytest.raises(engine.GrlbwtError) as e:
            ctx.parse2bwt()
        assert "parse phase not finished" in str(e.value)
        ctx.par_phase()
        ctx.parse2bwt()
        with pytest.raises(engine.GrlbwtError) as e:
            ctx.parse2bwt()
        assert e.value.code == cases.EINVAL and "once per text" in str(e.value)
        ctx.ind_phase()
        with pytest.raises(engine.GrlbwtError) as e:
            ctx.infer_lvl_bwt()
        assert e.value.code == cases.EINVAL and "built already" in str(e.value)
        assert ctx.result_bytes() == cases.expected(b"ACGT\nAC\n")[0]
