#!/usr/bin/env python3
"""What removing or keeping strings of an image (grlbwt_select_*) costs on the device, against what it replaces.

Steps, one after the other, each a child process under a time limit of its own; a step that fails ends the run:
  1gb    the 1 GB workload (6,622,517 x 150 bp reads sampled from a 33 Mbp genome)
  10gb   the headline workload (66,225,166 x 150 bp reads from a 330 Mbp genome)
  long   4 random ACGT strings of 8 M cells: one string dropped, per string and through checkpoints
A read step builds the image, then for "drop 1 %", "drop 50 %" and "keep 1 %" of the strings (seeded choice) times
grlbwt_select_create + grlbwt_select_emit, compares the result byte for byte with the image grlbwt_build makes of the reduced text,
and times what the call replaces: grlbwt_invert_image of the image plus grlbwt_build of the reduced text (the cut of the text, a
row gather on the device, is timed too and reported apart).  With the profile on it reports the marking walk alone
(select.mark) against the length walk of the per-string inverter over the same strings (inv.lengths under GRLBWT_INVERT=runs,
RunInvertLenFn): for that pair all strings but one are dropped, so both walk the same chains but one.  The two differ by the
atomic OR per step and by the launch (tickets against one lane per string).

Usage: python tools/gpu_image_select.py [--out profiles/image_select/select.txt] [--steps 1gb,long]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"1gb": (6622517, 33000000, 300), "10gb": (66225166, 330000000, 900), "long": (4, 8 << 20, 240)}      # strings, genome or length, time limit (s)
READ_LEN = 150


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def build_image(torch, engine, dist, lib, t):
    torch.cuda.synchronize()
    with engine.Context(0, 0, lib) as ctx:
        t0 = time.perf_counter()
        ctx.attach_device(t.data_ptr(), t.numel(), 1, keepalive=t)
        ctx.build()
        dt = time.perf_counter() - t0
        nb, runs = ctx.result_size()
        img = dist._view(ctx.result_device_ptr(), nb, torch.device("cuda:0")).clone()
        torch.cuda.synchronize()
    return img, runs, dt


def select(torch, engine, ctx, img, ids, **kw):
    """(output image, info, seconds of create, seconds of emit)"""
    sel, t_create = timed(torch, lambda: engine.ImageSelect(ctx, img.data_ptr(), img.numel(), 1, ids.data_ptr(), ids.numel(), **kw))
    info = sel.info()
    out = torch.empty(info["out_bytes"], dtype=torch.uint8, device="cuda:0")
    _, t_emit = timed(torch, lambda: sel.emit(out.data_ptr(), out.numel()))
    sel.close()
    return out, info, t_create, t_emit


def step_reads(name, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import dist, engine, workloads
    reads, genome, _ = STEPS[name]
    lib = g.build_hip()
    text = workloads.sampled_reads_torch(reads, READ_LEN, genome, seed=20260003, device="cuda:0")
    rows = text.view(reads, READ_LEN + 1)
    n = text.numel()
    say("== %s: %d reads of %d bp, %d cells (%s)" % (name, reads, READ_LEN, n, torch.cuda.get_device_name(0)))
    build_image(torch, engine, dist, lib, text)                        # (warm: the arena is backed, the kernels are loaded)
    img, runs, t_build = build_image(torch, engine, dist, lib, text)
    say("grlbwt_build of the whole collection: %.3f s, %d runs, image %d bytes" % (t_build, runs, img.numel()))
    gen = torch.Generator(device="cuda:0").manual_seed(20261019)
    perm = torch.randperm(reads, generator=gen, device="cuda:0")
    one, half = reads // 100, reads // 2
    cases = [("drop 1 %", perm[:one], False), ("drop 50 %", perm[:half], False), ("keep 1 %", perm[:one], True)]
    with engine.Context(0, 0, lib) as ctx:
        text_out = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        select(torch, engine, ctx, img, perm[:1000].to(torch.int64).contiguous())      # warm-up of the new kernels
        for label, chosen, keep in cases:
            ids = chosen.to(torch.int64).contiguous()
            out, info, t_create, t_emit = select(torch, engine, ctx, img, ids, keep=keep)
            # what the call replaces: invert, cut, build
            _, t_inv = timed(torch, lambda: ctx.invert_image(img.data_ptr(), img.numel(), 1, text_out.data_ptr(), n))
            assert torch.equal(text_out, text), "the inversion does not give the text back"
            mask = torch.zeros(reads, dtype=torch.bool, device="cuda:0")
            mask[ids] = True
            reduced, t_cut = timed(torch, lambda: text_out.view(reads, READ_LEN + 1)[mask if keep else ~mask].reshape(-1).contiguous())
            want, runs2, t_b2 = build_image(torch, engine, dist, lib, reduced)
            same = out.numel() == want.numel() and bool(torch.equal(out, want))
            say("%-9s: %d strings listed, %d rows marked, longest walk %d; %d -> %d runs; select create %.3f s + emit %.3f s = %.3f s; %s the build of the reduced text"
                % (label, info["n_listed"], info["rows_marked"], info["longest_walk"], info["n_runs_in"], info["n_runs_out"], t_create, t_emit,
                   t_create + t_emit, "byte for byte" if same else "DIFFERS FROM"))
            say("           replaced: invert %.3f s + cut %.3f s + build of %d cells %.3f s = %.3f s (%.1fx); scratch %d bytes (%.2f per row), held %d bytes"
                % (t_inv, t_cut, reduced.numel(), t_b2, t_inv + t_cut + t_b2, (t_inv + t_cut + t_b2) / (t_create + t_emit), info["scratch_bytes"],
                   info["scratch_bytes"] / n, info["held_bytes"]))
            if not same:
                sys.exit("the selected image differs from the built one")
            del reduced, want, out, mask
        # the marking walk against the length walk of the per-string inverter, over the same strings but one
        ids = perm[1:].to(torch.int64).contiguous()
        ctx.profile_enable(True)
        out, info, t_create, t_emit = select(torch, engine, ctx, img, ids)
        prof = ctx.profile()
        ctx.profile_enable(False)
        mark = prof.get("select.mark", (0, 0.0, 0))
        os.environ["GRLBWT_INVERT"] = "runs"
        os.environ["GRLBWT_QUIET_ENV"] = "1"
        ctx.profile_enable(True)
        ctx.invert_image(img.data_ptr(), img.numel(), 1, text_out.data_ptr(), n)
        prof2 = ctx.profile()
        ctx.profile_enable(False)
        del os.environ["GRLBWT_INVERT"]
        lens = prof2.get("inv.lengths", (0, 0.0, 0))
        say("marking walk alone: select.mark %.3f ms over %d strings (%d lanes, %d refills); inv.lengths (RunInvertLenFn, one lane per string) %.3f ms over %d strings: %.2fx"
            % (mark[1], info["n_listed"], info["walk_lanes"], info["lane_refills"], lens[1], reads, mark[1] / lens[1] if lens[1] else float("nan")))
        say("a byte per row with plain stores instead of the atomic OR: not measured (the product keeps the bit-vector form)")


def step_long(name, say):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import dist, engine
    k, ln, _ = STEPS[name]
    lib = g.build_hip()
    gen = torch.Generator(device="cuda:0").manual_seed(20261019)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda:0")
    body = acgt[torch.randint(0, 4, (k, ln), generator=gen, device="cuda:0")]
    text = torch.cat([body, torch.full((k, 1), 10, dtype=torch.uint8, device="cuda:0")], dim=1).reshape(-1).contiguous()
    say("== %s: %d strings of %d cells, %d cells (%s)" % (name, k, ln, text.numel(), torch.cuda.get_device_name(0)))
    img, runs, t_build = build_image(torch, engine, dist, lib, text)
    ids = torch.tensor([1], dtype=torch.int64, device="cuda:0")
    reduced = text.view(k, ln + 1)[[0, 2, 3]].reshape(-1).contiguous()
    want, _, t_b2 = build_image(torch, engine, dist, lib, reduced)
    say("grlbwt_build: whole %.3f s (%d runs), without string 1 %.3f s" % (t_build, runs, t_b2))
    with engine.Context(0, 0, lib) as ctx:
        for label, kw in (("checkpoints, sample_bits 8", dict(checkpoints=True, sample_bits=8)), ("checkpoints, sample_bits 4", dict(checkpoints=True, sample_bits=4)),
                          ("per string", dict())):
            if kw:
                select(torch, engine, ctx, img, ids, **kw)              # warm-up
            out, info, t_create, t_emit = select(torch, engine, ctx, img, ids, **kw)
            same = out.numel() == want.numel() and bool(torch.equal(out, want))
            say("drop 1 of %d, %-27s: create %.3f s + emit %.3f s; longest walk %d steps, %d checkpoints, %d jump rounds, scratch %d bytes; %s the build of the reduced text"
                % (k, label, t_create, t_emit, info["longest_walk"], info["n_checkpoints"], info["jump_rounds"], info["scratch_bytes"],
                   "byte for byte" if same else "DIFFERS FROM"))
            if not same:
                sys.exit("the selected image differs from the built one")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_select", "select.txt"))
    ap.add_argument("--steps", default="1gb,long")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    args = ap.parse_args()
    if args.step:
        def say(s):
            print(s, flush=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")
        return step_long(args.step, say) if args.step == "long" else step_reads(args.step, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("grlbwt_select_*: removing and keeping strings of an image on read collections and on long strings (tools/gpu_image_select.py)\n")
    for name in args.steps.split(","):
        limit = STEPS[name][2]
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--out", args.out])
        if rc != 0:
            with open(args.out, "a") as f:
                f.write("step %s ended with status %d: nothing further was run\n" % (name, rc))
            sys.exit(rc)


if __name__ == "__main__":
    main()
