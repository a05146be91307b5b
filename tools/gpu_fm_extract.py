#!/usr/bin/env python3
"""What grlbwt_fm_extract costs, on the `long` collection of tools/gpu_checkpointed_walks.py (4 random ACGT strings of 8 M cells,
built on the device, seeded).

ONE leg per invocation (--leg).  The tool has no time limit of its own: every leg is its own command under `timeout`, the
commands chained with `&&` so that the first failure ends the run:
    timeout -k 10 200 python tools/gpu_fm_extract.py --leg whole &&
    timeout -k 10 200 python tools/gpu_fm_extract.py --leg hits --append &&
    timeout -k 10 200 python tools/gpu_fm_extract.py --leg build --append
Legs:
  whole   (a) one range per whole string against grlbwt_invert_image_checkpointed of the same image at the same sample_bits
          (4, 8 and the default), three alternated runs each: median, fastest, slowest, and their ratio.  Both walk the same
          segments; the extraction adds its plan and two binary searches per piece and stores cell by cell.
  hits    (b) on the same index 1 M ranges of 150 cells at located hits (random rows, located, the range clamped by its string's
          end), against the whole inversion of (a): what a user paid before for the same answer.
  build   (c) grlbwt_fm_create and index_bytes with and without GRLBWT_FM_EXTRACT at sample_bits 4 and 8.
Every extracted cell is compared with the text.

Usage: python tools/gpu_fm_extract.py --leg whole|hits|build [--out profiles/fm_extract/extract.txt] [--append] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 3
LEGS = ("whole", "hits", "build")


def make_text(torch, small):
    g = torch.Generator(device="cuda:0").manual_seed(20261019)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda:0")
    k, ln = 4, (8 << 20) // (16 if small else 1)
    body = acgt[torch.randint(0, 4, (k, ln), generator=g, device="cuda:0")]
    text = torch.cat([body, torch.full((k, 1), 10, dtype=torch.uint8, device="cuda:0")], dim=1).reshape(-1).contiguous()
    torch.cuda.synchronize()
    return text, k, ln


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[0], ts[-1]


def u64(torch, values):
    return torch.tensor(values, dtype=torch.int64, device="cuda:0")


def extract(torch, fm, s, b, e, out, offs):
    t0 = time.perf_counter()
    n = fm.extract(s.data_ptr(), b.data_ptr(), e.data_ptr(), s.numel(), 1, out.data_ptr(), out.numel(), offs.data_ptr())
    return time.perf_counter() - t0, n


def invert(ctx, img, nb, out, n, bits):
    out.zero_()
    t0 = time.perf_counter()
    got, info = ctx.invert_image_checkpointed(img, nb, 1, out.data_ptr(), n, sample_bits=bits)
    assert got == n
    return time.perf_counter() - t0


def leg_whole(torch, engine, ctx, img, nb, text, k, ln, say, args):
    n = text.numel()
    out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    s, b, e = u64(torch, list(range(k))), u64(torch, [0] * k), u64(torch, [-1] * k)
    offs = torch.zeros(k + 1, dtype=torch.int64, device="cuda:0")
    for bits in (4, 8, 0):
        with engine.FmIndex(ctx, img, nb, locate=True, checkpoints=True, sample_bits=bits, extract=True) as fm:
            extract(torch, fm, s, b, e, out, offs)                # warm-up
            invert(ctx, img, nb, out, n, bits)
            tx, ti = [], []
            for _ in range(REPS):
                out.zero_()
                dt, got = extract(torch, fm, s, b, e, out, offs)
                assert got == n and torch.equal(out, text), "the extracted strings are not the text"
                tx.append(dt)
                ti.append(invert(ctx, img, nb, out, n, bits))
                assert torch.equal(out, text)
            xi = fm.extract_info()
            mx, mi = stats(tx), stats(ti)
            say("bits %2d: extract of %d whole strings median %.4f s min %.4f max %.4f; checkpointed inversion median %.4f s min %.4f max %.4f; ratio %.2f"
                "  (pieces %d, steps %d, lanes %d, refills %d, samples %d)"
                % ((fm.walk_info()["sample_bits"], k) + mx + mi + (mx[0] / mi[0], xi["n_pieces"], xi["walk_steps"], xi["walk_lanes"], xi["lane_refills"], xi["n_samples"])))


def leg_hits(torch, engine, ctx, img, nb, text, k, ln, say, args):
    n = text.numel()
    n_hits, width = (1 << 20) // (16 if args.small else 1), 150
    g = torch.Generator(device="cpu").manual_seed(7)
    rows = torch.randint(0, n, (n_hits,), generator=g).to("cuda:0").contiguous()
    full = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(n_hits * width, dtype=torch.uint8, device="cuda:0")
    offs = torch.zeros(n_hits + 1, dtype=torch.int64, device="cuda:0")
    for bits in (4, 8):
        with engine.FmIndex(ctx, img, nb, locate=True, checkpoints=True, sample_bits=bits, extract=True) as fm:
            s = torch.zeros(n_hits, dtype=torch.int64, device="cuda:0")
            o = torch.zeros(n_hits, dtype=torch.int64, device="cuda:0")
            fm.locate(rows.data_ptr(), n_hits, engine.UINT64_MAX, s.data_ptr(), o.data_ptr())
            e = o + width
            extract(torch, fm, s, o, e, out, offs)
            tx, ti = [], []
            for _ in range(REPS):
                dt, got = extract(torch, fm, s, o, e, out, offs)
                tx.append(dt)
                ti.append(invert(ctx, img, nb, full, n, bits))
            # against the text: range i is text[at, at + its length)
            lens = offs[1:] - offs[:-1]
            at = s * (ln + 1) + o
            assert bool((lens == torch.clamp(ln + 1 - o, max=width)).all()) and int(offs[-1]) == got
            src = torch.repeat_interleave(at - offs[:-1], lens) + torch.arange(got, device="cuda:0")
            assert torch.equal(out[:got], text[src]), "the extracted hits are not the text"
            xi = fm.extract_info()
            mx, mi = stats(tx), stats(ti)
            say("bits %2d: extract of %d ranges of %d cells (%d cells) median %.4f s min %.4f max %.4f; whole inversion median %.4f s: %.2fx of it"
                "  (pieces %d, steps %d, lanes %d, refills %d)"
                % ((bits, n_hits, width, got) + mx + (mi[0], mx[0] / mi[0], xi["n_pieces"], xi["walk_steps"], xi["walk_lanes"], xi["lane_refills"])))


def leg_build(torch, engine, ctx, img, nb, text, k, ln, say, args):
    for bits in (4, 8):
        res = {}
        for ext in (False, True):
            ts = []
            for r in range(REPS + 1):                             # (the first is the warm-up)
                t0 = time.perf_counter()
                fm = engine.FmIndex(ctx, img, nb, locate=True, checkpoints=True, sample_bits=bits, extract=ext)
                ts.append(time.perf_counter() - t0)
                info = fm.info()
                xb = fm.extract_info()["extract_bytes"] if ext else 0
                fm.close()
            res[ext] = (stats(ts[1:]), info["index_bytes"], xb)
        (a, ab, _), (b, bb, xb) = res[False], res[True]
        assert bb == ab + xb
        say("bits %2d: create without the bit median %.4f s min %.4f max %.4f, %d bytes; with it median %.4f s min %.4f max %.4f, %d bytes (%d added, %.2f %%)"
            % ((bits,) + a + (ab,) + b + (bb, xb, 100.0 * xb / ab)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_extract", "extract.txt"))
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it")
    ap.add_argument("--small", action="store_true", help="a collection of a sixteenth of the size")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    torch.zeros(1, device="cuda:0")
    import __graft_entry__ as g
    from grlbwt_amd import engine
    lib = g.build_hip()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    f = open(args.out, "a" if args.append else "w")

    def say(s):
        print(s, flush=True)
        f.write(s + "\n")
        f.flush()

    if not args.append:
        say("grlbwt_fm_extract on %s%s" % (torch.cuda.get_device_name(0), " (--small)" if args.small else ""))
    text, k, ln = make_text(torch, args.small)
    n = text.numel()
    t0 = time.perf_counter()
    with engine.Context(0, 0, lib) as ctx:
        ctx.attach_device(text.data_ptr(), n, 1, keepalive=text)
        ctx.build()
        nb, runs = ctx.result_size()
        img = ctx.result_device_ptr()
        say("== %s: %d strings of %d cells, %d cells, %d runs" % (args.leg, k, ln, n, runs))
        {"whole": leg_whole, "hits": leg_hits, "build": leg_build}[args.leg](torch, engine, ctx, img, nb, text, k, ln, say, args)
    say("leg %s: %.1f s" % (args.leg, time.perf_counter() - t0))


if __name__ == "__main__":
    main()
