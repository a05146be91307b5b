#!/usr/bin/env python3
"""The price of wide symbols, and the figures behind the regimes of the alphabet compaction.

Steps, each a child process of its own under a time limit of its own; the first one that fails ends the script:
  wide     workloads.wide_tokens (64-bit values, -a 8): the per-kernel lines of the compaction (alpha.*) and the whole build
  ranks    the same collection given as the ranks of its values with -a 4 (no compaction: the path every narrow collection takes),
           with this tree's library or -- the comparison of the two -- with the built checkout of the parent commit that
           --baseline-root names (its library through its own host mirror)
  regimes  the compaction alone (grlbwt_alphabet_compact_device) on uniformly drawn values, for alphabets on both sides of each
           threshold and with the sorting regime forced (GRLBWT_ALPHA_TABLE_BITS=2)
Usage: python tools/gpu_wide_alphabet.py [--cells 128000000] [--baseline-root DIR] [--out profiles/r07/wide_alphabet.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _collection(n_cells):
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("wide_workloads", os.path.join(ROOT, "grlbwt_amd", "workloads.py"))
    workloads = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(workloads)
    cells, ids, table = workloads.wide_tokens(n_cells, 1000, 65000, 64, with_ids=True)
    present = np.bincount(ids, minlength=len(table)) > 0
    rank_of = np.cumsum(present) - 1                       # ids that occur, in id order ...
    order = np.argsort(table[present], kind="stable")      # ... and their values' order
    dense = np.empty(len(order), dtype=np.uint32)
    dense[order] = np.arange(len(order), dtype=np.uint32)
    return cells, dense[rank_of[ids]], int(present.sum())


def _timed_builds(tensor, w, reps):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine
    lib = g.build_hip()
    out = {}
    with engine.Context(0, 0, lib) as ctx:
        def step():
            ctx.attach_device(tensor.data_ptr(), tensor.numel(), w, keepalive=tensor)
            ctx.build()
        step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["build_ms"] = ts
        out["image_bytes"] = ctx.result_size()[0]
        import hashlib
        out["image_md5"] = hashlib.md5(ctx.result_bytes()).hexdigest()
        c = ctx.counters()
        out["t_stats_ms"] = c["t_stats"] * 1e3
        ctx.profile_enable(True)
        ctx.attach_device(tensor.data_ptr(), tensor.numel(), w, keepalive=tensor)
        prof = ctx.profile()
        out["load_kernels"] = {k: {"launches": v[0], "ms": v[1], "bytes": v[2]} for k, v in prof.items() if k.startswith(("alpha.", "stats."))}
        out["memory"] = ctx.memory_usage()
    return out


def step_wide(args):
    import numpy as np
    import torch
    cells, _, sigma = _collection(args.cells)
    t = torch.from_numpy(cells.view(np.int64)).to("cuda:0")
    res = _timed_builds(t, 8, args.reps)
    res.update(cells=int(cells.size), distinct=sigma, floor_bytes=int(cells.size) * 12)
    return res


def step_ranks(args):
    import numpy as np
    import torch
    if args.baseline_root:
        sys.path.insert(0, os.path.abspath(args.baseline_root))      # its __graft_entry__ and grlbwt_amd in front of this tree's
    cells, ranks, sigma = _collection(args.cells)
    t = torch.from_numpy(ranks.view(np.int32)).to("cuda:0")
    res = _timed_builds(t, 4, args.reps)
    res.update(cells=int(cells.size), distinct=sigma, library="baseline checkout" if args.baseline_root else "this tree")
    return res


def step_regimes(args):
    import torch
    import __graft_entry__ as g
    from grlbwt_amd import engine
    lib = g.build_hip()
    n = args.cells
    rows = []
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(20260007)
    for w in (8, 4):
        for sigma, forced in ((5, False), (1024, False), (2048, False), (4096, False), (4097, False), (8192, False), (8193, False), (65536, False), (262144, False), (500000, False),
                              (600000, False), (65536, True)):
            if w == 8:
                table = torch.randint(-2 ** 63, 2 ** 63 - 1, (sigma,), dtype=torch.int64, device="cuda:0", generator=gen)
                table = torch.where(table >= -5, table - 5, table)            # nothing above 2^64 - 5
            else:
                table = torch.randint(-2 ** 31, 2 ** 31 - 1, (sigma,), dtype=torch.int32, device="cuda:0", generator=gen)
            cells = table[torch.randint(0, sigma, (n,), device="cuda:0", generator=gen)].contiguous()
            ranks = torch.empty(n, dtype=torch.int32, device="cuda:0")
            values = torch.empty(sigma, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            if forced:
                os.environ["GRLBWT_ALPHA_TABLE_BITS"] = "2"
            with engine.Context(0, 0, lib) as ctx:
                ctx.alphabet_compact(cells.data_ptr(), n, w, ranks.data_ptr(), values.data_ptr(), sigma)
                ctx.profile_enable(True)
                t0 = time.perf_counter()
                k = ctx.alphabet_compact(cells.data_ptr(), n, w, ranks.data_ptr(), values.data_ptr(), sigma)
                wall = (time.perf_counter() - t0) * 1e3
                prof = ctx.profile()
            os.environ.pop("GRLBWT_ALPHA_TABLE_BITS", None)
            sites = {}
            for name, (c, ms, _) in prof.items():
                if name.startswith("alpha."):
                    s = name.partition("#")[0]
                    sites[s] = round(sites.get(s, 0.0) + ms, 3)
            rows.append({"cell_bytes": w, "cells": n, "drawn": sigma, "distinct": k, "forced_sort": forced, "wall_ms": round(wall, 3), "kernel_ms": sites})
            print(rows[-1], flush=True)
            del cells, ranks, values, table
    return {"rows": rows}


STEPS = {"wide": (step_wide, 600), "ranks": (step_ranks, 600), "regimes": (step_regimes, 420)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "wide_alphabet.json"))
    ap.add_argument("--steps", default="wide,ranks,regimes")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        res = STEPS[args.step][0](args)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    out = {"cells": args.cells, "steps": {}}
    for name in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--cells", str(args.cells), "--reps", str(args.reps)]
        if args.baseline_root:
            cmd += ["--baseline-root", args.baseline_root]
        print("== step %s" % name, flush=True)
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1])
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: stopping" % (name, STEPS[name][1]))
            return 1
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-3000:] + p.stderr[-3000:])
            print("step %s failed (exit %d): stopping" % (name, p.returncode))
            return 1
        out["steps"][name] = json.loads(lines[-1][7:])
        print(json.dumps(out["steps"][name])[:2000], flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
