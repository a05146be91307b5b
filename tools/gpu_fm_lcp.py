#!/usr/bin/env python3
"""grlbwt_fm_lcp on images of read collections and of long strings: the two forms of a pass against each other -- the fused kernel
(prim::LcpRound, GRLBWT_LCP_ROUND unset) and the generic primitives (GRLBWT_LCP_ROUND=plain).

ONE leg per invocation (--leg); the tool starts no child process.  Every leg is its own command under `timeout`, the commands
chained with `&&` so that the first failure ends the run:
    timeout -k 10 300 python tools/gpu_fm_lcp.py --leg reads101 &&
    timeout -k 10 500 python tools/gpu_fm_lcp.py --leg reads1g --append &&
    timeout -k 10 300 python tools/gpu_fm_lcp.py --leg long --append
Legs (grlbwt_amd/workloads.py, tools/gpu_checkpointed_walks.py):
  reads101  1,000,000 x 100 bp uniform reads (101 MB), uncapped and at max_lcp = 32
  reads1g   6,622,517 x 150 bp reads sampled from a 33 Mbp genome (1 GB), uncapped and at max_lcp = 32
  long      4 random ACGT strings of 8 M cells, at max_lcp = 32 (uncapped their passes are as many as their longest repeat)

Per leg: build the image, make one index, and per setting: a warm-up call of each form, then the two forms take turns inside
each repetition.  A call with max_lcp = 1 runs no pass: its median is what a call costs besides its passes (the scratch, the
F-order run-start bit-vector, the first bits), and (call - that) / passes is the time of a pass.  Written per form: the passes,
the median / fastest / slowest call, the milliseconds per pass, the bytes a pass must move --
    (B and S read and written: 4 x n / 8) + (the RankCells: 16 x n / 64) + (12 or 24 bytes per run: key and slf)
-- and the rate achieved against them.  Nothing about the rate is fixed in advance.

Checked on the way: both forms write the same values and histograms; the histogram's rows and the capped rows add up to n; the
distinct 1-mers are the symbols of the text.

Usage: python tools/gpu_fm_lcp.py --leg reads101|reads1g|long [--out profiles/fm_lcp/lcp.txt] [--append] [--reps 5] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = (("fused", None), ("plain", "plain"))
LEGS = ("reads101", "reads1g", "long")


def set_form(value):
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    if value is None:
        os.environ.pop("GRLBWT_LCP_ROUND", None)
    else:
        os.environ["GRLBWT_LCP_ROUND"] = value


def make_text(torch, workloads, leg, small):
    div = 16 if small else 1
    if leg == "reads101":
        return "101 MB uniform reads", workloads.uniform_reads_torch(1000000 // div, 100, device="cuda:0")
    if leg == "reads1g":
        return "1 GB sampled reads", workloads.sampled_reads_torch(6622517 // div, 150, 33000000 // div, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(20261019)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda:0")
    body = acgt[torch.randint(0, 4, (4, (8 << 20) // div), generator=g, device="cuda:0")]
    sep = torch.full((4, 1), 10, dtype=torch.uint8, device="cuda:0")
    return "4 strings of 8 M cells", torch.cat([body, sep], dim=1).reshape(-1).contiguous()


def bytes_per_pass(n, runs, idx_bytes):
    return 4 * (n // 8) + 16 * (n // 64) + runs * (12 if idx_bytes == 4 else 24)


def measure(leg, args, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
    lib = g.build_hip()
    name, text = make_text(torch, workloads, leg, args.small)
    torch.cuda.synchronize()
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), text.numel(), 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        image_ptr = ctx.result_device_ptr()              # stays valid while the context holds this build
        set_form(None)
        with engine.FmIndex(ctx, image_ptr, nb) as fm:
            info = fm.info()
            n, R = info["n_syms"], info["n_runs"]
            need = bytes_per_pass(n, R, info["idx_bytes"])
            say("== %s: %d cells, %d strings, %d runs, image %d bytes, index %d bytes, idx_bytes %d; a pass must move %d bytes"
                % (name, n, info["n_strings"], R, nb, info["index_bytes"], info["idx_bytes"], need))
            out = torch.zeros(n, dtype=torch.int16, device="cuda:0")

            def call(form, max_lcp, w):
                set_form(form)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ra, su = fm.lcp(max_lcp, w, out.data_ptr())
                return time.perf_counter() - t0, ra, su

            base = {}
            for label, form in FORMS:                        # a call without a pass
                call(form, 1, 1)
                base[label] = statistics.median(call(form, 1, 1)[0] for _ in range(args.reps))
                say("max_lcp 1 (no pass) %-5s: median %9.3f ms" % (label, base[label] * 1e3))
            settings = ((32, 1),) if leg == "long" else ((0, 2), (32, 1))
            for max_lcp, w in settings:
                what = "max_lcp %d, %d-byte values" % (max_lcp, w) if max_lcp else "uncapped, %d-byte values" % w
                ref, infos = None, {}
                for label, form in FORMS:                    # warm-up, and both forms write the same
                    _, ra, su = call(form, max_lcp, w)
                    infos[label] = fm.lcp_info()
                    got = (out.view(torch.uint8)[:n * w].clone(), ra, su)
                    if ref is None:
                        ref = got
                    assert torch.equal(ref[0], got[0]) and (ref[1] == got[1]).all() and (ref[2] == got[2]).all(), "the forms disagree"
                li = infos["fused"]
                assert li == infos["plain"], infos
                assert int(ref[1].sum()) + li["n_capped"] == n and int(ref[2][0]) == info["n_strings"]
                assert engine.FmIndex.distinct_kmers(ref[1], ref[2], 1) == info["sigma"] - 1
                times = {label: [] for label, _ in FORMS}
                for _ in range(args.reps):
                    for label, form in FORMS:
                        times[label].append(call(form, max_lcp, w)[0])
                set_form(None)
                say("%s: %d passes, largest value %d, %d rows capped, scratch %d bytes, tile %d rows"
                    % (what, li["passes"], li["max_lcp"], li["n_capped"], li["scratch_bytes"], li["tile_rows"]))
                per = {}
                for label, _ in FORMS:
                    ts = sorted(times[label])
                    med = statistics.median(ts)
                    per[label] = (med - base[label]) / max(li["passes"], 1)
                    say("  %-5s: call median %10.3f ms  min %10.3f  max %10.3f  -> %8.4f ms per pass, %7.1f GB/s of the bytes a pass must move"
                        % (label, med * 1e3, ts[0] * 1e3, ts[-1] * 1e3, per[label] * 1e3, need / per[label] / 1e9 if per[label] > 0 else 0.0))
                spread = max(max(times[l]) - min(times[l]) for l, _ in FORMS) / max(li["passes"], 1)
                verdict = "fused" if per["fused"] < per["plain"] - spread else "plain" if per["plain"] < per["fused"] - spread else "within the spread"
                say("  per pass: fused %.4f ms, plain %.4f ms, spread of the repetitions %.4f ms: %s" % (per["fused"] * 1e3, per["plain"] * 1e3, spread * 1e3, verdict))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_lcp", "lcp.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
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
        say("grlbwt_fm_lcp: a pass as the fused kernel (default) and as the generic primitives (GRLBWT_LCP_ROUND=plain) on %s%s"
            % (torch.cuda.get_device_name(0), "; collections cut to a sixteenth (--small)" if args.small else ""))
    measure(args.leg, args, say)


if __name__ == "__main__":
    main()
