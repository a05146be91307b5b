"""What tests/test_call_order_sim.py and tests/test_call_order_gpu.py share: the call-order contract of the stage-wise C API
(the table beside the phase declarations of include/grlbwt_hip.h), checked against a model of that table written here in plain
Python.  The model shares no code with the engine: it knows the five states, the six calls and the number of parsing rounds the
oracle needs, nothing else.

A sequence is checked call by call (the return code, parse_round's `done`, parse_phase's rounds), then grlbwt_result_size must
succeed exactly when the model says DONE, and a grlbwt_build afterwards must give the oracle's image: a refused or no-op call
never changes what the following calls produce."""
import ctypes as C
import functools
import itertools

import numpy as np

from grlbwt_amd import engine, workloads
from oracle import oracle
from tests import base_case_cases
from tests import wide_check as wc

OK, EINVAL = 0, -22
CALLS = ("parse_round", "parse_phase", "induce_first", "induce_level", "induce_phase", "build")
LOADED, PARTLY, PARSED, INDUCING, DONE = "LOADED", "PARTLY PARSED", "PARSED", "INDUCING", "DONE"
RATIO = base_case_cases.RATIO


def model(seq, rounds, start=(LOADED, 0, 0)):
    """The table of include/grlbwt_hip.h.  -> ([(kind, code, out) of every call], (state, rounds parsed, level)): kind is
    "advance", "noop" or "refused"; out is parse_round's `done`, parse_phase's round count (None where a build parsed on its
    own and may have stopped at a level of short strings), None for the other calls."""
    state, parsed, level = start
    steps = []
    for call in seq:
        parsing = state in (LOADED, PARTLY)
        kind, out = "advance", None
        if call == "parse_round":
            if parsing:
                parsed += 1
                state = PARSED if parsed == rounds else PARTLY
            else:
                kind = "noop"
            out = state not in (LOADED, PARTLY)
        elif call == "parse_phase":
            if parsing:
                parsed, state = rounds, PARSED
            else:
                kind = "noop"
            out = parsed
        elif call == "induce_first":
            if state == PARSED:
                state, level = INDUCING, rounds
            else:
                kind = "refused"
        elif call == "induce_level":
            if state == INDUCING:
                level -= 1
                state = DONE if level == 0 else INDUCING
            else:
                kind = "refused"
        elif call in ("induce_phase", "build"):
            if call == "induce_phase" and parsing:
                kind = "refused"
            elif state == DONE:
                kind = "noop"
            else:
                if parsing:
                    parsed = None
                state, level = DONE, 0
        else:
            raise ValueError(call)
        steps.append((kind, EINVAL if kind == "refused" else OK, out))
    return steps, (state, parsed, level)


def all_sequences(max_len=3):
    """every sequence of 1 to max_len calls: 6 + 36 + 216 = 258 for three"""
    return [s for k in range(1, max_len + 1) for s in itertools.product(CALLS, repeat=k)]


def start_of(state, rounds):
    """a (state, rounds parsed, level) the model can start from"""
    return {LOADED: (LOADED, 0, 0), PARTLY: (PARTLY, 1, 0), PARSED: (PARSED, rounds, 0), INDUCING: (INDUCING, rounds, rounds),
            DONE: (DONE, rounds, 0)}[state]


def idle_transitions(rounds):
    """every (state, call) the table refuses or makes a no-op: 18 of them"""
    return {(st, c): model([c], rounds, start_of(st, rounds))[0][0][0]
            for st in (LOADED, PARTLY, PARSED, INDUCING, DONE) for c in CALLS
            if model([c], rounds, start_of(st, rounds))[0][0][0] != "advance"}


# The device module's sequences: together they hold every refused and every no-op transition (assert_covers); the two faults this
# contract closed -- a second induce_first, an induce_phase that is not the first induction call -- among them.
DEVICE_SEQUENCES = (
    ("induce_first", "induce_level", "induce_phase", "build"),
    ("parse_round", "induce_first", "induce_level", "induce_phase", "build"),
    ("parse_phase", "parse_round", "parse_phase", "induce_level", "induce_first"),
    ("parse_phase", "induce_first", "parse_round", "parse_phase", "induce_first", "induce_phase"),
    ("build", "parse_round", "parse_phase", "induce_first", "induce_level", "induce_phase", "build"),
    ("parse_phase", "induce_phase", "induce_phase", "induce_first"),
    ("parse_phase", "induce_first", "induce_level", "induce_first", "build", "induce_level"),
    ("parse_round", "build", "build"),
    ("parse_phase", "induce_first", "induce_level", "induce_phase", "induce_level"),
    ("parse_round", "parse_round", "parse_phase", "induce_first", "build", "induce_first"),
    ("parse_phase", "build", "parse_round"),
    ("parse_phase", "induce_first", "induce_phase", "induce_phase"),
    ("build", "induce_first", "induce_first", "build"),
    ("build", "induce_phase", "induce_phase"),
    ("parse_phase", "induce_first", "induce_first", "induce_level"),
    ("parse_phase", "induce_first", "induce_level", "induce_phase", "induce_phase"),
    ("induce_level", "parse_round", "induce_level", "parse_phase", "induce_level"),
    ("parse_phase", "induce_phase", "build", "parse_phase"),
    ("parse_round", "induce_phase", "parse_phase", "induce_phase"),
    ("build",),
)


def assert_covers(sequences, rounds):
    """the sequences pass through every transition of idle_transitions"""
    seen = set()
    for seq in sequences:
        state = (LOADED, 0, 0)
        for call in seq:
            steps, nxt = model([call], rounds, state)
            if steps[0][0] != "advance":
                seen.add((state[0], call))
            state = nxt
    missing = set(idle_transitions(rounds)) - seen
    assert not missing, sorted(missing)


# ---- inputs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_reads():
    """reads of 20x coverage, small enough for the whole enumeration on the stand-in: four rounds or more at the oracle, and a
    plain build stops at a level of short strings (both asserted by the test that uses them)"""
    return workloads.sampled_reads(500, 100, 5000, seed=11).tobytes()


@functools.lru_cache(maxsize=None)
def small_tokens():
    return workloads.zipf_tokens(40000, doc_len=200, vocab=5000).tobytes()


@functools.lru_cache(maxsize=None)
def expected(data, cell_bytes=1):
    """(image, rounds) of the oracle, computed once per input"""
    return base_case_cases.expected(data, cell_bytes)


def wide_expected(w=8):
    """(cells, image) of the wide-symbol collection of tests/base_case_cases.py: built on ranks, records of more than 8 bytes"""
    cells = base_case_cases.wide(w)
    return cells, _wide_image(w)


@functools.lru_cache(maxsize=None)
def _wide_image(w):
    return wc.oracle_on_ranks(base_case_cases.wide(w), w)


# ---- driving the C API ---------------------------------------------------------------------------------------------------
def drive(ctx, call):
    """(return code, out) of one stage call through the C ABI, no exception in between"""
    L, h = ctx.L, ctx._h
    if call == "parse_round":
        info, done = engine.RoundInfo(), C.c_int(-1)
        return L.grlbwt_parse_round(h, C.byref(info), C.byref(done)), done.value
    if call == "parse_phase":
        n = C.c_int(-1)
        return L.grlbwt_parse_phase(h, C.byref(n)), n.value
    if call == "induce_first":
        return L.grlbwt_induce_first(h), None
    if call == "induce_level":
        lvl, info = C.c_int(-1), engine.LevelInfo()
        return L.grlbwt_induce_level(h, C.byref(lvl), C.byref(info)), lvl.value
    if call == "induce_phase":
        return L.grlbwt_induce_phase(h), None
    if call == "build":
        return L.grlbwt_build(h), None
    raise ValueError(call)


def last_error(ctx):
    return ctx.L.grlbwt_last_error(ctx._h).decode()


def result_size_code(ctx):
    nb, nr = C.c_uint64(), C.c_uint64()
    return ctx.L.grlbwt_result_size(ctx._h, C.byref(nb), C.byref(nr))


def check_call(ctx, call, step, rounds, where):
    """one call against the model's (kind, code, out)"""
    kind, code, out = step
    rc, got = drive(ctx, call)
    assert rc == code, "%s: %s returned %d, the model says %d (%s)" % (where, call, rc, code, last_error(ctx))
    if kind == "refused":
        msg = last_error(ctx)
        assert msg, "%s: %s refused without a message" % (where, call)
        return msg
    if call == "parse_round":
        assert got == int(out), "%s: parse_round says done = %d" % (where, got)
    if call == "parse_phase":
        assert (got == out) if out is not None else (1 <= got <= rounds), "%s: parse_phase says %d rounds of %d" % (where, got, rounds)
    return None


def check_sequence(ctx, seq, rounds, want):
    """`seq` on a context whose text has just been loaded"""
    steps, (state, _, _) = model(seq, rounds)
    where = ", ".join(seq)
    for call, step in zip(seq, steps):
        check_call(ctx, call, step, rounds, where)
    rc = result_size_code(ctx)
    assert rc == (OK if state == DONE else EINVAL), "%s: result_size returned %d in %s" % (where, rc, state)
    rc, _ = drive(ctx, "build")
    assert rc == OK, "%s: the build afterwards returned %d (%s)" % (where, rc, last_error(ctx))
    got = ctx.result_bytes()
    assert got == want, "%s: the image afterwards differs (%d vs %d bytes)" % (where, len(got), len(want))


def check_sequences(lib, sequences, data, cell_bytes, flags, rounds, want):
    """every sequence on one context, the text loaded again in front of each"""
    with engine.Context(0, flags, lib) as ctx:
        for seq in sequences:
            ctx.upload(data, cell_bytes)
            check_sequence(ctx, seq, rounds, want)


def rounds_of_plain_build(lib, data, cell_bytes=1, flags=0):
    """the rounds par_phase() reports after build()"""
    with engine.Context(0, flags, lib) as ctx:
        ctx.upload(data, cell_bytes)
        ctx.build()
        return ctx.par_phase()


# ---- the hook of parity.check_stagewise ----------------------------------------------------------------------------------
def state_of(ctx, rounds):
    """the engine's state as the inspection calls show it (none of them is a stage call)"""
    if result_size_code(ctx) == OK:
        return DONE
    L, h = ctx.L, ctx._h
    if L.grlbwt_level_info_get(h, 0, C.byref(engine.LevelInfo())) == OK:
        return INDUCING
    n = 0
    while L.grlbwt_round_info_get(h, n, C.byref(engine.RoundInfo())) == OK:
        n += 1
    return PARSED if n == rounds else PARTLY if n else LOADED


class IdleCalls:
    """between=...: fires every call the table refuses or makes a no-op in the state the context is in, and counts them"""

    def __init__(self, rounds):
        self.rounds, self.fired = rounds, {}

    def __call__(self, ctx):
        state = state_of(ctx, self.rounds)
        for call in CALLS:
            steps, after = model([call], self.rounds, start_of(state, self.rounds))
            if steps[0][0] == "advance":
                continue
            assert after[0] == state
            check_call(ctx, call, steps[0], self.rounds, "in " + state)
            self.fired[(state, call)] = self.fired.get((state, call), 0) + 1
        assert state_of(ctx, self.rounds) == state


# ---- DONE is idempotent ----------------------------------------------------------------------------------------------------
def check_idempotent_done(lib, data, cell_bytes, want, flags=0):
    """build, then build / induce_phase / parse_round again: the image stays where it is and as it is"""
    with engine.Context(0, flags, lib) as ctx:
        ctx.upload(data, cell_bytes)
        ctx.build()
        p, b, size = ctx.result_device_ptr(), ctx.result_bytes(), ctx.result_size()
        assert b == want, "rl_bwt differs (%d vs %d bytes)" % (len(b), len(want))
        ctx.build()
        ctx.ind_phase()
        _, done = ctx.parse_round()
        assert done
        assert ctx.result_device_ptr() == p and ctx.result_size() == size
        assert ctx.result_bytes() == b


# ---- one context, text after text ------------------------------------------------------------------------------------------
ILL_FORMED = b"AC\nGT"          # the last cell is not the smallest


def check_no_text(ctx, earlier):
    """a context without a text: EINVAL from stats, build and result, and a message that is not the earlier failure's"""
    L, h = ctx.L, ctx._h
    for rc in (L.grlbwt_get_stats(h, C.byref(engine.Stats())), drive(ctx, "build")[0], result_size_code(ctx)):
        assert rc == EINVAL, rc
        assert earlier not in last_error(ctx), last_error(ctx)


def check_context_reuse(lib, reads, tokens, flags=0):
    want_reads, want_tokens = expected(reads)[0], expected(tokens, 2)[0]
    cells, want_wide = wide_expected(8)
    with engine.Context(0, flags, lib) as ctx:
        ctx.upload(reads, 1)
        ctx.build()
        first = ctx.result_bytes()
        assert first == want_reads and ctx.alphabet_size() == 0
        ctx.upload(tokens, 2)
        ctx.build()
        assert ctx.result_bytes() == want_tokens
        try:
            ctx.upload(ILL_FORMED, 1)
        except engine.IllFormedInput as e:
            assert "ill formed" in str(e)
        else:
            raise AssertionError("an ill-formed text was accepted")
        check_no_text(ctx, "ill formed")
        ctx.upload(cells.tobytes(), 8)
        assert ctx.alphabet_size() > 0
        ctx.build()
        assert ctx.result_bytes() == want_wide
        ctx.upload(reads, 1)
        assert ctx.alphabet_size() == 0
        ctx.build()
        assert ctx.result_bytes() == first


# ---- a refused build, then the same build again ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def borrowed_reads():
    """the reads of test_borrowed_text_that_changes_after_attach_is_refused: large enough for the sampled direct index"""
    return workloads.sampled_reads(40000, 150, 300000, seed=77)


def aligned_copy(a):
    """a copy of a uint8 array that starts on a 16-byte boundary (grlbwt_text_attach_device asks for that)"""
    raw = np.empty(a.size + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    out = raw[off:off + a.size]
    out[:] = a
    return out
