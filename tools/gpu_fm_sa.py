#!/usr/bin/env python3
"""grlbwt_fm_sa -- the document array and the suffix array of every row in one walk per string (form 0) or per checkpoint segment
(form 1) -- against grlbwt_fm_locate over rows 0 .. n - 1 on the SAME index, the call it replaces for "every row".

ONE leg per invocation (--leg); the tool starts no child process.  Every leg is its own command under `timeout`, the commands
chained with `&&` so that the first failure ends the run:
    timeout -k 10 400 python tools/gpu_fm_sa.py --leg reads101 &&
    timeout -k 10 300 python tools/gpu_fm_sa.py --leg long --append
Legs (grlbwt_amd/workloads.py, tools/gpu_checkpointed_walks.py):
  reads101  1,000,000 x 100 bp uniform reads (101 MB): form 0 (an index without checkpoints), form 1 at sample_bits 4 and 8
  long      4 random ACGT strings of 8 M cells: form 1 at sample_bits 4 and 8.  Form 0 and the locate-all of an index without
            checkpoints are not run there: 8 M dependent steps per string, minutes by design.

Per index: one warm-up of each call, then the calls take turns inside each repetition -- locate-all, the arrays at 8-byte entries
(what locate writes) and at the narrowest widths that fit.  Written per call: the median / fastest / slowest time, the LF steps
the call reports (locate-all: the steps by the located offsets, or by the distance to the next checkpoint) and steps per second,
and the ratio of the locate-all median to the call's.  Nothing about the ratio is fixed in advance.

Checked on the way: the 8-byte arrays equal what locate-all wrote, byte for byte; the narrow arrays equal them narrowed.

Usage: python tools/gpu_fm_sa.py --leg reads101|long [--out profiles/fm_sa/sa.txt] [--append] [--reps 3] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("reads101", "long")


def make_text(torch, workloads, leg, small):
    div = 16 if small else 1
    if leg == "reads101":
        return "101 MB uniform reads", workloads.uniform_reads_torch(1000000 // div, 100, device="cuda:0"), (None, 4, 8)
    g = torch.Generator(device="cuda:0").manual_seed(20261019)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda:0")
    body = acgt[torch.randint(0, 4, (4, (8 << 20) // div), generator=g, device="cuda:0")]
    sep = torch.full((4, 1), 10, dtype=torch.uint8, device="cuda:0")
    return "4 strings of 8 M cells", torch.cat([body, sep], dim=1).reshape(-1).contiguous(), (4, 8)


def narrowest(v):
    return next(w for w in (1, 2, 4, 8) if w == 8 or v < 1 << (8 * w))


def measure(leg, args, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    lib = g.build_hip()
    name, text, forms = make_text(torch, workloads, leg, args.small)
    torch.cuda.synchronize()
    DT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        for bits in forms:
            kw = {} if bits is None else dict(checkpoints=True, sample_bits=bits)
            with engine.FmIndex(ctx, image_ptr, nb, locate=True, **kw) as fm:
                info = fm.info()
                n, k = info["n_syms"], info["n_strings"]
                say("== %s, %s: %d rows, %d strings, %d runs, index %d bytes, idx_bytes %d"
                    % (name, "form 0 (no checkpoints)" if bits is None else "form 1 (sample_bits %d, %d checkpoints)" % (bits, fm.walk_info()["n_checkpoints"]),
                       n, k, info["n_runs"], info["index_bytes"], info["idx_bytes"]))
                rows = torch.arange(n, dtype=torch.int64, device="cuda:0")
                ls, lo = torch.empty(n, dtype=torch.int64, device="cuda:0"), torch.empty(n, dtype=torch.int64, device="cuda:0")
                s8, o8 = torch.empty_like(ls), torch.empty_like(lo)

                def locate_all():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fm.locate(rows.data_ptr(), n, engine.UINT64_MAX, ls.data_ptr(), lo.data_ptr())
                    return time.perf_counter() - t0

                def arrays(ws, s, wo, o):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fm.suffix_array(0, None, ws, s.data_ptr(), wo, o.data_ptr())
                    return time.perf_counter() - t0

                locate_all()                                  # warm-up, and the values everything is held to
                ws, wo = narrowest(k - 1), narrowest(int(lo.max()))
                sn, on = torch.empty(n, dtype=DT[ws], device="cuda:0"), torch.empty(n, dtype=DT[wo], device="cuda:0")
                calls = (("locate-all (8, 8)", locate_all), ("arrays (8, 8)", lambda: arrays(8, s8, 8, o8)),
                         ("arrays (%d, %d)" % (ws, wo), lambda: arrays(ws, sn, wo, on)))
                steps = {}
                for label, fn in calls[1:]:
                    fn()
                    steps[label] = fm.sa_info()
                assert torch.equal(s8, ls) and torch.equal(o8, lo), "the arrays differ from locate-all"
                assert torch.equal(sn, ls.to(DT[ws])) and torch.equal(on, lo.to(DT[wo])), "the narrow arrays differ from locate-all"
                loc_steps = int(lo.sum()) if bits is None else None      # (with checkpoints a row stops at the first one on its way: not counted)
                times = {label: [] for label, _ in calls}
                for _ in range(args.reps):
                    for label, fn in calls:
                        times[label].append(fn())
                base = statistics.median(times[calls[0][0]])
                for label, _ in calls:
                    ts = sorted(times[label])
                    med = statistics.median(ts)
                    if label in steps:
                        si = steps[label]
                        st = si["walk_steps"]
                        extra = ", longest walk %d, %d lanes, %d refills, scratch %d bytes" % (si["longest_walk"], si["walk_lanes"], si["lane_refills"], si["scratch_bytes"])
                    else:
                        st, extra = loc_steps, ""
                    rate = "%d LF steps, %8.1f M steps/s" % (st, st / med / 1e6) if st is not None else "LF steps not counted by the call"
                    say("  %-18s: median %10.3f ms  min %10.3f  max %10.3f  %s  locate-all / this = %6.2f%s"
                        % (label, med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, rate, base / med, extra))
                del rows, ls, lo, s8, o8, sn, on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_sa", "sa.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a sixteenth of every collection")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    torch.zeros(1, device="cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = open(args.out).read().splitlines() if args.append and os.path.exists(args.out) else []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not lines:
        say("grlbwt_fm_sa against grlbwt_fm_locate over all rows of the same index on %s%s"
            % (torch.cuda.get_device_name(0), "; collections cut to a sixteenth (--small)" if args.small else ""))
    measure(args.leg, args, say)


if __name__ == "__main__":
    main()
