#!/usr/bin/env python3
"""What the checkpointed LF walks are worth: grlbwt_invert_image_checkpointed against grlbwt_invert_image under
GRLBWT_INVERT=runs (one lane per string), and the locate index with and without GRLBWT_FM_CHECKPOINTS.

Collections (built on the device, seeded):
  long     4 random ACGT strings of 8 M cells
  repeats  16 strings of 2 M cells: copies of one 1 500-cell random unit, 1 cell in 1 000 changed, independently per string
  reads    1 M random ACGT strings of 150 cells

ONE leg per invocation (--leg).  The tool has no time limit of its own: every leg is its own command under `timeout`, the
commands chained with `&&` so that the first failure ends the run:
    timeout -k 10 400 python tools/gpu_checkpointed_walks.py --leg invert:long &&
    timeout -k 10 200 python tools/gpu_checkpointed_walks.py --leg invert:repeats --append && ...
Legs:
  invert:<collection>   per-string inverter and the checkpointed one at sample_bits 6, 8, 10, 12, three alternated runs each:
                        median, fastest, slowest; longest_segment, jump_rounds, scratch bytes; the checkpointed form at the
                        default sample_bits with one lane per checkpoint (GRLBWT_WALK_LANES above the checkpoint count: no
                        lane takes a second ticket) against the refilling launch
  index:<collection>    create with and without checkpoints, locate of random rows.  On `long` and `repeats` the unsampled
                        create is one run and the unsampled locate takes 1 024 rows (a row walks to the start of its string:
                        millions of dependent steps); the index with checkpoints locates 1 M rows everywhere
  stores:<collection>   the two store forms of the write walk, plain cell stores and aligned 8-byte words of collected cells (the
                        form the library takes for u8 / u16 cells), three alternated runs each at sample_bits 6 and 8.  Needs the
                        development build (tools/build_dev.sh), whose GRLBWT_DEV_WALK_STORES=cells switch brings the plain
                        form back: --lib tools/_build/libgrlbwt_dev.so
Every inversion is compared with the text, every located position with the unsampled index's on the rows both located.

Usage: python tools/gpu_checkpointed_walks.py --leg KIND:COLLECTION [--out profiles/checkpointed_walks/walks.txt] [--append] [--small] [--lib PATH]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BITS = (6, 8, 10, 12)
REPS = 3
LEGS = [k + ":" + c for k in ("invert", "index", "stores") for c in ("long", "repeats", "reads")]


def make_text(torch, name, small):
    g = torch.Generator(device="cuda:0").manual_seed(20261019)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda:0")
    div = 16 if small else 1

    def rand(*shape):
        return acgt[torch.randint(0, 4, shape, generator=g, device="cuda:0")]

    if name == "long":
        k, ln = 4, (8 << 20) // div
        body = rand(k, ln)
    elif name == "repeats":
        k, ln, unit = 16, (2 << 20) // div, 1500
        body = rand(unit).repeat(-(-ln // unit))[:ln].repeat(k, 1)
        hit = torch.rand((k, ln), generator=g, device="cuda:0") < 0.001
        other = acgt[torch.randint(0, 4, (k, ln), generator=g, device="cuda:0")]
        body = torch.where(hit, other, body)
    else:
        k, ln = (1 << 20) // div, 150
        body = rand(k, ln)
    text = torch.cat([body, torch.full((k, 1), 10, dtype=torch.uint8, device="cuda:0")], dim=1).reshape(-1).contiguous()
    torch.cuda.synchronize()
    return text, k, ln


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[0], ts[-1]


def leg_invert(torch, engine, lib, name, args, say):
    text, k, ln = make_text(torch, name, args.small)
    n = text.numel()
    out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), n, 1, keepalive=text)
        t0 = time.perf_counter()
        ctx.build()
        t_build = time.perf_counter() - t0
        nb, runs = ctx.result_size()
        img = ctx.result_device_ptr()
        say("== invert:%s: %d strings of %d cells, %d cells, %d runs, engine build %.3f s" % (name, k, ln, n, runs, t_build))

        def parent():
            os.environ["GRLBWT_INVERT"] = "runs"
            try:
                out.zero_()
                t0 = time.perf_counter()
                got = ctx.invert_image(img, nb, 1, out.data_ptr(), n)
                dt = time.perf_counter() - t0
            finally:
                del os.environ["GRLBWT_INVERT"]
            assert got == n and torch.equal(out, text), "the per-string inverter does not give the text back"
            return dt, None

        def checkpointed(bits, lanes=None):
            if lanes:
                os.environ["GRLBWT_WALK_LANES"] = str(lanes)
            try:
                out.zero_()
                t0 = time.perf_counter()
                got, info = ctx.invert_image_checkpointed(img, nb, 1, out.data_ptr(), n, sample_bits=bits)
                dt = time.perf_counter() - t0
            finally:
                os.environ.pop("GRLBWT_WALK_LANES", None)
            assert got == n and torch.equal(out, text), "the checkpointed inverter does not give the text back"
            return dt, info

        forms = [("per-string", parent)] + [("bits %2d" % b, (lambda b=b: checkpointed(b))) for b in BITS]
        times = {f: [] for f, _ in forms}
        infos = {}
        checkpointed(8)                                  # warm-up of the new kernels
        for _ in range(REPS):
            for f, fn in forms:
                dt, info = fn()
                times[f].append(dt)
                infos[f] = info
        base = stats(times["per-string"])
        for f, _ in forms:
            med, lo, hi = stats(times[f])
            i = infos[f]
            extra = "" if i is None else "  checkpoints %d, longest_segment %d, longest_chain %d, jump_rounds %d, lanes %d, refills %d, scratch %d bytes" % (
                i["n_checkpoints"], i["longest_segment"], i["longest_chain"], i["jump_rounds"], i["walk_lanes"], i["lane_refills"], i["scratch_bytes"])
            say("%-10s median %9.3f s  min %9.3f  max %9.3f  (%.2fx of per-string)%s" % (f, med, lo, hi, base[0] / med, extra))
        best = min(BITS, key=lambda b: stats(times["bits %2d" % b])[0])
        bm = stats(times["bits %2d" % best])
        say("fastest sample_bits %d: %.3f s against %.3f s per-string; spreads (max - min) %.3f s and %.3f s: %s"
            % (best, bm[0], base[0], bm[2] - bm[1], base[2] - base[1],
               "faster by more than the spread" if base[1] > bm[2] else "NOT faster by more than the spread"))
        # lane refill on and off at the default sample_bits
        t_on, t_off = [], []
        for _ in range(REPS):
            dt, i_on = checkpointed(0)
            t_on.append(dt)
            dt, i_off = checkpointed(0, lanes=1 << 40)
            t_off.append(dt)
        say("refill on  (default bits %d): median %.3f s min %.3f max %.3f, lanes %d refills %d" % ((i_on["sample_bits"],) + stats(t_on) + (i_on["walk_lanes"], i_on["lane_refills"])))
        say("refill off (one lane per checkpoint): median %.3f s min %.3f max %.3f, lanes %d refills %d" % (stats(t_off) + (i_off["walk_lanes"], i_off["lane_refills"])))


def leg_stores(torch, engine, lib, name, args, say):
    text, k, ln = make_text(torch, name, args.small)
    n = text.numel()
    out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), n, 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        img = ctx.result_device_ptr()
        say("== stores:%s: %d strings of %d cells, %d cells, %d runs (development build)" % (name, k, ln, n, runs))

        def call(bits, form):
            if form == "plain":
                os.environ["GRLBWT_DEV_WALK_STORES"] = "cells"
            try:
                out.zero_()
                ctx.profile_enable(True)
                t0 = time.perf_counter()
                got, info = ctx.invert_image_checkpointed(img, nb, 1, out.data_ptr(), n, sample_bits=bits)
                dt = time.perf_counter() - t0
                prof = ctx.profile()
                ctx.profile_enable(False)
            finally:
                os.environ.pop("GRLBWT_DEV_WALK_STORES", None)
            assert got == n and torch.equal(out, text), "the %s form does not give the text back" % form
            kern = "cp.write_packed" if form == "packed" else "cp.write"
            assert kern in prof, (form, sorted(prof))
            return dt, prof[kern][1]

        call(8, "plain")
        call(8, "packed")
        for bits in (6, 8):
            t = {"plain": [], "packed": []}
            kms = {"plain": [], "packed": []}
            for _ in range(REPS):
                for form in ("plain", "packed"):
                    dt, ms = call(bits, form)
                    t[form].append(dt)
                    kms[form].append(ms)
            for form in ("plain", "packed"):
                say("bits %2d %-6s stores: call median %.4f s min %.4f max %.4f; write kernel median %.3f ms min %.3f max %.3f"
                    % ((bits, form) + stats(t[form]) + stats(kms[form])))


def leg_index(torch, engine, lib, name, args, say):
    text, k, ln = make_text(torch, name, args.small)
    n = text.numel()
    long_strings = name != "reads"
    n_rows = (1 << 20) // (16 if args.small else 1)
    g = torch.Generator(device="cpu").manual_seed(7)
    rows = torch.randint(0, n, (n_rows,), generator=g).to("cuda:0").contiguous()
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), n, 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        img = ctx.result_device_ptr()
        say("== index:%s: %d strings of %d cells, %d cells, %d runs" % (name, k, ln, n, runs))

        def locate(fm, r):
            s = torch.zeros(r.numel(), dtype=torch.int64, device="cuda:0")
            o = torch.zeros(r.numel(), dtype=torch.int64, device="cuda:0")
            t0 = time.perf_counter()
            fm.locate(r.data_ptr(), r.numel(), engine.UINT64_MAX, s.data_ptr(), o.data_ptr())
            return time.perf_counter() - t0, s, o

        t_plain = []
        for _ in range(1 if long_strings else REPS):
            t0 = time.perf_counter()
            plain = engine.FmIndex(ctx, img, nb, locate=True)
            t_plain.append(time.perf_counter() - t0)
            if len(t_plain) < (1 if long_strings else REPS):
                plain.close()
        say("create without checkpoints: median %.3f s min %.3f max %.3f (%d run%s), %d bytes"
            % (stats(t_plain) + (len(t_plain), "" if len(t_plain) == 1 else "s", plain.info()["index_bytes"])))
        few = rows[:1024].contiguous() if long_strings else rows
        dt, s0, o0 = locate(plain, few)
        say("locate without checkpoints: %d rows in %.3f s" % (few.numel(), dt))
        for b in BITS:
            ts = []
            for r in range(REPS):
                t0 = time.perf_counter()
                fm = engine.FmIndex(ctx, img, nb, locate=True, checkpoints=True, sample_bits=b)
                ts.append(time.perf_counter() - t0)
                if r + 1 < REPS:
                    fm.close()
            wi = fm.walk_info()
            tl = []
            for _ in range(REPS):
                dt, s1, o1 = locate(fm, rows)
                tl.append(dt)
            assert torch.equal(s1[:few.numel()], s0) and torch.equal(o1[:few.numel()], o0), "the two indexes locate differently"
            at = s1 * (ln + 1) + o1
            assert bool((at >= 0).all()) and bool((at < n).all())
            say("bits %2d: create median %.3f s min %.3f max %.3f, %d bytes (%d of samples), longest_segment %d, jump_rounds %d; locate %d rows median %.4f s min %.4f max %.4f"
                % ((b,) + stats(ts) + (fm.info()["index_bytes"], wi["sample_bytes"], wi["longest_segment"], wi["jump_rounds"], n_rows) + stats(tl)))
            fm.close()
        plain.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpointed_walks", "walks.txt"))
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it")
    ap.add_argument("--small", action="store_true", help="collections of a sixteenth of the size")
    ap.add_argument("--lib", default=None, help="another build of the device library (the stores legs: tools/_build/libgrlbwt_dev.so)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    torch.zeros(1, device="cuda:0")
    import __graft_entry__ as g
    from grlbwt_amd import engine
    lib = os.path.abspath(args.lib) if args.lib else g.build_hip()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    f = open(args.out, "a" if args.append else "w")

    def say(s):
        print(s, flush=True)
        f.write(s + "\n")
        f.flush()

    if not args.append:
        say("checkpointed LF walks on %s%s" % (torch.cuda.get_device_name(0), " (--small)" if args.small else ""))
    kind, name = args.leg.split(":")
    t0 = time.perf_counter()
    {"invert": leg_invert, "index": leg_index, "stores": leg_stores}[kind](torch, engine, lib, name, args, say)
    say("leg %s: %.1f s" % (args.leg, time.perf_counter() - t0))


if __name__ == "__main__":
    main()
