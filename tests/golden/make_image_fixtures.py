#!/usr/bin/env python3
"""Generates tests/golden/ref_image_consumers.json -- run in the BUILD container (needs the reference tree).

The images of tests/image_cases.py (made by numpy, not by the engine: empty records, repeated symbols, wide headers, giant
lengths) are written to a temporary file each and given to the reference's own programs from oracle/_ref/ (oracle/Makefile
target `ref`): grl2plain with and without the null replacement, grlbwt2rle, bwt_stats (sb = 1) and split_runs for every
(bits, block) of the case.  Recorded: md5/size of the image and of every output, the printed statistics parsed as in
ref_consumers.json.  Only these data go into git.

* The giant-length cases are not given to grl2plain (their plain form is 2^32 bytes and more).
* The programs run under an address-space limit of 4 GiB: split_runs allocates 8 * block_size bytes of counters, so a block
  of 2^31 (16 GiB) or 2^38 (2 TiB) ends it with std::bad_alloc on any machine, the same way everywhere.
* Where a program does not end with status 0 (split_runs asserts on block 0 and, on some inputs, on its own block count)
  the entry holds "reference": "aborts" and the program's message; the test then checks the engine's output by definition.
  At most one in six of the split settings with a block may be of that kind: asserted here.

Usage:  python tests/golden/make_image_fixtures.py        (prints the number of settings the reference aborted on)
"""
import hashlib
import json
import os
import resource
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle  # noqa: E402
from tests import image_cases as ic  # noqa: E402
from tests.golden.make_ref_fixtures import parse_bwt_stats, parse_split  # noqa: E402

OUT = os.path.join(HERE, "ref_image_consumers.json")
AS_LIMIT = 4 << 30


def md5(b):
    return hashlib.md5(b).hexdigest()


def _limit():
    resource.setrlimit(resource.RLIMIT_AS, (AS_LIMIT, AS_LIMIT))
    resource.setrlimit(resource.RLIMIT_CORE, (0, 0))


def run_ref(prog, args, cwd):
    """(stdout, None) or (None, last line the program wrote before it died)"""
    p = subprocess.run([oracle.ref_prog(prog)] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, preexec_fn=_limit)
    if p.returncode == 0:
        return p.stdout, None
    msg = [l for l in (p.stderr or "").strip().splitlines() if l.strip()]
    msg = msg[-1].strip() if msg else "status %d" % p.returncode
    return None, msg.replace(cwd + "/", "").replace(oracle.REF_DIR + "/", "").replace(oracle.REFERENCE_ROOT + "/", "")


def reference_outputs(case, td):
    """What the reference's programs make of one case: the dictionary stored in the fixture."""
    blob = case.image()
    f = os.path.join(td, "in.rl_bwt")
    with open(f, "wb") as fh:
        fh.write(blob)
    rd = lambda name: open(os.path.join(td, name), "rb").read()
    c = {"name": case.name, "sb": case.sb, "fb": case.fb, "runs": case.R, "n": case.n, "image_md5": md5(blob), "image_size": len(blob)}
    if not case.giant:
        out, err = run_ref("grl2plain", [f, "plain"], td)
        assert err is None, (case.name, err)
        c["plain_md5"], c["plain_size"] = md5(rd("plain")), len(rd("plain"))
        out, err = run_ref("grl2plain", [f, "plain35", "35"], td)
        assert err is None, (case.name, err)
        c["plain_null35_md5"] = md5(rd("plain35"))
    out, err = run_ref("grlbwt2rle", [f, "rle"], td)
    assert err is None, (case.name, err)
    c["syms_md5"], c["len_md5"] = md5(rd("rle.syms")), md5(rd("rle.len"))
    c["syms_size"], c["len_size"] = len(rd("rle.syms")), len(rd("rle.len"))
    if case.sb == 1 and case.R:                # bwt_stats indexes 256-entry tables by the symbol; no run at all: it reads past its vector
        out, err = run_ref("bwt_stats", [f], td)
        assert err is None, (case.name, err)
        c["bwt_stats"] = parse_bwt_stats(out)
        if case.R < 10:                        # its decile index ceil(r*0.9..) runs past the vector
            c["bwt_stats"]["deciles"] = None
    c["split_runs"] = []
    for bits, block in case.splits:
        e = {"bits": bits, "block": block}
        if os.path.exists(os.path.join(td, "split.out")):
            os.remove(os.path.join(td, "split.out"))
        out, err = run_ref("split_runs", [f, bits, block, "split.out"], td)      # argv order of the code: file bits n output
        if err is not None:
            e["reference"], e["message"] = "aborts", err
        else:
            ob = rd("split.out")
            e.update({"out_md5": md5(ob), "out_size": len(ob)})
            e.update(parse_split(out))
        c["split_runs"].append(e)
    return c


def main():
    assert oracle.build_ref(force=True), "needs the reference tree (build container)"
    fixtures = {"_about": "reference scripts/{grl2plain,grlbwt2rle,bwt_stats,split_runs}.cpp (oracle/Makefile ref) run on the images "
                          "of tests/image_cases.py; generated by tests/golden/make_image_fixtures.py", "cases": []}
    with_block = aborted = aborted0 = 0
    for case in ic.CASES:
        with tempfile.TemporaryDirectory() as td:
            c = reference_outputs(case, td)
        fixtures["cases"].append(c)
        for e in c["split_runs"]:
            bad = e.get("reference") == "aborts"
            if e["block"]:
                with_block += 1
                aborted += bad
            else:
                aborted0 += bad
        print(case.name, case.R, case.n, [(e["bits"], e["block"], e.get("runs_after", e.get("message"))) for e in c["split_runs"]])
    print("split settings with a block: %d, the reference aborted on %d of them (cap: one in six); on %d settings with block 0"
          % (with_block, aborted, aborted0))
    assert aborted * 6 <= with_block, "too many split settings are checked by definition only: choose other seeds"
    with open(OUT, "w") as f:
        json.dump(fixtures, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
