#!/usr/bin/env python3
"""grlbwt_fm_repeats on images of read collections, uncapped and at max_len = 32: the whole table (lo, count, len, split).

ONE leg per invocation (--leg).  The only child process is the host's cc for --route-b, run before the GPU is opened.  Every leg is
its own command under `timeout`, chained with `&&`:
    timeout -k 10 400 python tools/gpu_fm_repeats.py --leg reads101 --lib tools/_build/libgrlbwt_dev.so --route-b &&
    timeout -k 10 600 python tools/gpu_fm_repeats.py --leg reads1g --lib tools/_build/libgrlbwt_dev.so --route-b --append
Legs (grlbwt_amd/workloads.py, as tools/gpu_fm_kmers.py; `long` as tools/gpu_fm_extract.py):
  reads101  1,000,000 x 100 bp uniform reads (101 MB)
  reads1g   6,622,517 x 150 bp reads sampled from a 33 Mbp genome (1 GB)
  long      4 random ACGT strings of 8 M cells, at max_len = 32 only

Per leg and max_len: a sizing call (no arrays), then the filling call timed `--reps` times; with a development library (--lib, built
by tools/build_dev.sh) the tile kernels and the generic form (GRLBWT_DEV_REPEAT_SEARCH=f) take turns inside each repetition and must
write the same bytes.  One more call of each form runs under the library's profile: the kernels' times, grouped into the LCP
passes, the tree build, the search (heads, counting, selection) and the emit (for_each_set_bit in both forms).

--route-b: the route without this call, timed once: grlbwt_fm_lcp (max_lcp = max_len + 1 where there is one) into a device array
of 4-byte values, the array downloaded, and the textbook stack walk over it on the host (tools/repeat_stack_walk.c, compiled with
the host's cc into tools/_build/): right-maximal repeats only, no left-maximality.  Its number of repeats must be n_repeats.

Usage: python tools/gpu_fm_repeats.py --leg reads101|reads1g|long [--lib LIB] [--route-b] [--out profiles/fm_repeats/repeats.txt]
                                      [--append] [--reps 3] [--small]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("reads101", "reads1g", "long")
GROUPS = (("lcp passes", ("lcp.",)), ("tree", ("repeat.minima",)), ("emit", ("repeat.emit",)), ("search", ("repeat.",)))


def set_form(value):
    os.environ["GRLBWT_QUIET_ENV"] = "1"
    if value is None:
        os.environ.pop("GRLBWT_DEV_REPEAT_SEARCH", None)
    else:
        os.environ["GRLBWT_DEV_REPEAT_SEARCH"] = value


def make_text(torch, workloads, leg, small):
    div = 16 if small else 1
    if leg == "reads101":
        return "101 MB uniform reads", workloads.uniform_reads_torch(1000000 // div, 100, device="cuda:0")
    if leg == "reads1g":
        return "1 GB sampled reads", workloads.sampled_reads_torch(6622517 // div, 150, 33000000 // div, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(20261019)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda:0")
    body = acgt[torch.randint(0, 4, (4, (8 << 20) // div), generator=g, device="cuda:0")]
    text = torch.cat([body, torch.full((4, 1), 10, dtype=torch.uint8, device="cuda:0")], dim=1).reshape(-1).contiguous()
    return "4 strings of 8 M cells", text


def grouped(prof):
    out = {g: 0.0 for g, _ in GROUPS}
    for name, (_, ms, _) in prof.items():
        for g, prefixes in GROUPS:
            if any(name.startswith(p) for p in prefixes):
                out[g] += ms
                break
    return out


def stack_walk_lib():
    src, out = os.path.join(ROOT, "tools", "repeat_stack_walk.c"), os.path.join(ROOT, "tools", "_build", "librepeat_stack_walk.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", out, src])
    lib = ctypes.CDLL(out)
    lib.repeat_stack_walk.restype = ctypes.c_uint64
    lib.repeat_stack_walk.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return lib


def route_b(torch, np, fm, n, max_len, top, walk, say):
    """top: the largest value the array can hold (the stack holds strictly ascending values: top + 2 entries at the most)"""
    lcp = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    stack = np.zeros(2 * (top + 3), dtype=np.uint64)
    torch.cuda.synchronize()                             # (the library runs on its own stream: torch's fills come first)
    t0 = time.perf_counter()
    fm.lcp(max_len + 1 if max_len else 0, 4, lcp.data_ptr(), want_hist=False)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host = lcp.cpu().numpy()
    t2 = time.perf_counter()
    got = walk.repeat_stack_walk(host.ctypes.data, n, 1, max_len if max_len else 0xFFFFFFFF, stack.ctypes.data)
    t3 = time.perf_counter()
    assert int(host.max()) <= top
    say("  route without the call: lcp %.1f ms, download %.1f ms, stack walk on the host %.1f ms: %.1f ms, %d right-maximal repeats"
        % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3, got))
    return got


def measure(leg, args, say, walk):
    import numpy as np
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine, workloads
    lib = os.path.abspath(args.lib) if args.lib else g.build_hip()
    forms = (("tile", None), ("generic", "f")) if args.lib else (("tile", None),)
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
            n = info["n_syms"]
            say("== %s: %d cells, %d strings, %d runs, idx_bytes %d" % (name, n, info["n_strings"], runs, info["idx_bytes"]))
            for max_len in ((32,) if leg == "long" else (0, 32)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = fm.repeats_raw(max_len=max_len)
                t_size = time.perf_counter() - t0
                out = [torch.zeros(m, dtype=torch.int64, device="cuda:0") for _ in range(4)]

                def call(form):
                    set_form(form)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = fm.repeats_raw(max_len=max_len, lo_ptr=out[0].data_ptr(), count_ptr=out[1].data_ptr(), len_ptr=out[2].data_ptr(),
                                         split_ptr=out[3].data_ptr(), capacity=m)
                    torch.cuda.synchronize()
                    assert got == m
                    return time.perf_counter() - t0

                ref, infos = None, {}
                for label, form in forms:                    # warm-up, and both forms write the same
                    for o in out:
                        o.zero_()
                    call(form)
                    infos[label] = fm.repeat_info()
                    got = [o.clone() for o in out]
                    if ref is None:
                        ref = got
                    assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the forms disagree"
                lo, cnt, ln, sp = out
                assert bool((sp[1:] > sp[:-1]).all()) and bool((lo < sp).all()) and bool((sp < lo + cnt).all()) and bool((lo + cnt <= n).all())
                times = {label: [] for label, _ in forms}
                for _ in range(args.reps):
                    for label, form in forms:
                        times[label].append(call(form))
                ri = infos["tile"]
                say("max_len = %d: %d right-maximal repeats, %d of them maximal, longest %d, largest count %d; %d LCP passes; %d-byte values, "
                    "%d levels; %d searches left their tile; scratch %d bytes; sizing call %.1f ms"
                    % (max_len, ri["n_repeats"], ri["n_maximal"], ri["longest"], ri["largest_count"], ri["passes"], ri["value_bytes"],
                       ri["tree_levels"], ri["far_searches"], ri["scratch_bytes"], t_size * 1e3))
                for label, form in forms:
                    ctx.profile_enable(True)
                    call(form)
                    gr = grouped(ctx.profile())
                    ctx.profile_enable(False)
                    ts = sorted(times[label])
                    say("  %-7s: call median %9.2f ms  min %9.2f  max %9.2f | kernels: lcp passes %8.2f, tree %6.3f, search %8.3f, emit %8.3f ms"
                        % (label, statistics.median(ts) * 1e3, ts[0] * 1e3, ts[-1] * 1e3, gr["lcp passes"], gr["tree"], gr["search"], gr["emit"]))
                set_form(None)
                del out, ref, got
                if args.route_b:
                    assert route_b(torch, np, fm, n, max_len, ri["passes"] + 1, walk, say) == ri["n_repeats"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=LEGS)
    ap.add_argument("--lib", default=None, help="a development library (tools/build_dev.sh): the generic form is measured too")
    ap.add_argument("--route-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_repeats", "repeats.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a sixteenth of every collection")
    args = ap.parse_args()
    walk = stack_walk_lib() if args.route_b else None      # (cc runs before this process opens the GPU)
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
        say("grlbwt_fm_repeats: the whole table, the tile kernels (default) against the generic form (GRLBWT_DEV_REPEAT_SEARCH=f) on %s%s"
            % (torch.cuda.get_device_name(0), "; collections cut to a sixteenth (--small)" if args.small else ""))
    measure(args.leg, args, say, walk)


if __name__ == "__main__":
    main()
