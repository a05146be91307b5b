#!/usr/bin/env python3
"""What a refinement round of the image merge (grlbwt_merge_*) costs on the device, on read collections.

Two steps, one after the other, each a child process under a time limit of its own; a step that fails ends the run:
  1gb    the two halves of the 1 GB workload (6,622,517 x 150 bp reads sampled from a 33 Mbp genome)
  10gb   two 5 GB halves of the headline workload's generator (66,225,166 x 150 bp reads from a 330 Mbp genome)
A step builds the images of both halves and of the whole collection (the time of that build is the first baseline: what a
user does while the collection still fits one build), merges the halves with the profile on, compares the merged image with
the built one byte for byte on the device, and runs ONE round in the form that needs no kernel of its own
(GRLBWT_MERGE_ROUND=sort: gathered rank keys, prim::sort_pairs with a one-byte value; max_rounds = 1 ends the merge after it) --
the second baseline.  Written to --out: rounds, the three round kernels' milliseconds and rows changed per round (the library's
per-round log), bytes per row and round against the 6-byte bound, peak scratch, the totals.

Usage: python tools/gpu_image_merge.py [--out profiles/image_merge/rounds.txt] [--steps 1gb,10gb]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"1gb": (6622517, 33000000, 420), "10gb": (66225166, 330000000, 900)}      # reads, genome, time limit of the step (s)
READ_LEN = 150
KERNELS = ("merge.counts", "merge.hist", "merge.offsets", "merge.scatter", "merge.tile_scan")


def capture_stderr(fn):
    """fn() with the process's stderr (the library writes there) in a file; returns (fn's result or exception, the text)"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            try:
                res = fn()
            except Exception as e:      # noqa: BLE001 -- handed to the caller
                res = e
        finally:
            sys.stderr.flush()
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return res, f.read().decode(errors="replace")


def step(name, out):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import dist, engine, workloads
    reads, genome, _ = STEPS[name]
    lib = g.build_hip()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "a") as f:
            f.write(s + "\n")

    text = workloads.sampled_reads_torch(reads, READ_LEN, genome, seed=20260003, device="cuda:0")
    half = (reads // 2) * (READ_LEN + 1)
    torch.cuda.synchronize()
    say("== %s: %d reads of %d bp, %d cells; halves of %d and %d cells (%s)" % (name, reads, READ_LEN, text.numel(), half, text.numel() - half,
                                                                                 torch.cuda.get_device_name(0)))

    def build(t):
        torch.cuda.synchronize()                                       # (the engine's stream is its own: the cells must be complete)
        with engine.Context(0, 0, lib) as ctx:
            t0 = time.perf_counter()
            ctx.attach_device(t.data_ptr(), t.numel(), 1, keepalive=t)
            ctx.build()
            dt = time.perf_counter() - t0
            nb, runs = ctx.result_size()
            img = dist._view(ctx.result_device_ptr(), nb, dev).clone()
            torch.cuda.synchronize()
        return img, runs, dt

    img_a, runs_a, t_a = build(text[:half])
    img_b, runs_b, t_b = build(text[half:].clone())                   # (its own allocation: an attached text starts 16-byte aligned)
    build(text)                                                        # (warm: the arena is backed, the kernels are loaded)
    img_ab, runs_ab, t_ab = build(text)
    del text
    torch.cuda.empty_cache()
    say("grlbwt_build: A %.3f s (%d runs), B %.3f s (%d runs), A|B %.3f s (%d runs, image %d bytes)  <- baseline 1: the build of the concatenated text"
        % (t_a, runs_a, t_b, runs_b, t_ab, runs_ab, img_ab.numel()))
    with engine.Context(0, 0, lib) as ctx:
        def merge(max_rounds=0):
            t0 = time.perf_counter()
            mg = engine.ImageMerge(ctx, img_a.data_ptr(), img_a.numel(), img_b.data_ptr(), img_b.numel(), 1, max_rounds)
            return mg, time.perf_counter() - t0

        mg, _ = merge()                                                 # warm-up
        mg.close()
        ctx.profile_enable(True)
        (mg, t_merge), log = capture_stderr(merge)
        prof = ctx.profile()
        ctx.profile_enable(False)
        info = mg.info()
        n, R = info["n_syms_a"] + info["n_syms_b"], info["rounds"]
        outbuf = torch.empty(info["out_bytes"], dtype=torch.uint8, device=dev)
        t0 = time.perf_counter()
        mg.emit(outbuf.data_ptr(), outbuf.numel())
        t_emit = time.perf_counter() - t0
        same = outbuf.numel() == img_ab.numel() and bool(torch.equal(outbuf, img_ab))
        mg.close()
        say("merge: %d rounds, rows changed %d (%.2f per row), %d runs, %d bytes: %s the built image"
            % (R, info["rows_changed"], info["rows_changed"] / n, info["n_runs"], info["out_bytes"], "byte for byte" if same else "DIFFERS FROM"))
        say("merge: create %.3f s (load + all rounds + run count), emit %.3f s; held %d bytes (%.2f per row), peak scratch %d bytes (%.2f per row), tile %d rows"
            % (t_merge, t_emit, info["held_bytes"], info["held_bytes"] / n, info["scratch_bytes"], info["scratch_bytes"] / n, info["tile_rows"]))
        tot = {k: prof.get(k, (0, 0.0, 0)) for k in KERNELS}
        for k in KERNELS:
            say("  %-16s %5d launches %10.3f ms  (%.3f ms per round)" % (k, tot[k][0], tot[k][1], tot[k][1] / max(R, 1)))
        ms_round = sum(tot[k][1] for k in KERNELS) / max(R, 1)
        three = sum(tot[k][1] for k in ("merge.counts", "merge.hist", "merge.scatter")) / max(R, 1)
        # algorithmic bytes of a round: flags read by counts (twice: this interleave and the one before) and by scatter, ranks by hist
        # and scatter, flags written once -- the issue's 6 bytes per row, of which this form's hist reads no flags
        say("fused round: %.3f ms in the three kernels (%.3f with the offsets), %.2f G rows/s; the 6 bytes per row of the bound in that time are %.2f TB/s"
            % (three, ms_round, n / three / 1e6, 6 * n / three / 1e9))
        say("per round (rows changed; ms of counts / hist / scatter):")
        for m in re.finditer(r"merge round (\d+): rows changed (\d+); ms: counts ([\d.]+) hist ([\d.]+) scatter ([\d.]+)", log):
            say("  round %3s  %12s  %8s %8s %8s" % m.groups())
        # baseline 2: one round as gathered keys + the radix sort's pass over (key byte, flag byte)
        os.environ["GRLBWT_MERGE_ROUND"] = "sort"
        os.environ["GRLBWT_QUIET_ENV"] = "1"
        ctx.profile_enable(True)
        (res, log2) = capture_stderr(lambda: merge(1))
        prof2 = ctx.profile()
        ctx.profile_enable(False)
        del os.environ["GRLBWT_MERGE_ROUND"]
        assert isinstance(res, engine.GrlbwtError) and "not converged after 1 rounds" in str(res), res
        base = {k: v for k, v in prof2.items() if k.startswith("merge.") and k.split(".")[1] in ("bits", "bit_ranks", "keys", "sort", "changed")}
        for k in sorted(base):
            say("  %-20s %5d launches %10.3f ms" % (k, base[k][0], base[k][1]))
        ms_base = sum(v[1] for v in base.values())
        say("sort-form round (baseline 2): %.3f ms in its kernels, without the copies of the flags; the fused round takes %.2fx of that" % (ms_base, ms_round / ms_base))
        say("total: merge create + emit %.3f s against %.3f s for the build of the concatenated text (%.1fx)" % (t_merge + t_emit, t_ab, (t_merge + t_emit) / t_ab))
    if not same:
        sys.exit("the merged image differs from the built one")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_merge", "rounds.txt"))
    ap.add_argument("--steps", default="1gb,10gb")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("grlbwt_merge_*: rounds of the interleave refinement on read collections (tools/gpu_image_merge.py)\n")
    for name in args.steps.split(","):
        limit = STEPS[name][2]
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--out", args.out])
        if rc != 0:
            with open(args.out, "a") as f:
                f.write("step %s ended with status %d: nothing further was run\n" % (name, rc))
            sys.exit(rc)


if __name__ == "__main__":
    main()
