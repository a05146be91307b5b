"""`grlbwt --select IMAGE.rl_bwt (--drop IDS | --keep IDS) -o OUT`: the argument contract (no GPU), and the selected file against
the file the command line builds from the reduced text."""
import os
import subprocess

import numpy as np
import pytest

from tests import merge_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as g
    g.build_hip()
    return g.build_cli()


def run(cli, *args, cwd=None):
    p = subprocess.run([cli, *args], cwd=cwd, capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout, p.stderr


def test_cli_select_argument_contract(cli, tmp_path):
    img, ids, bad = tmp_path / "a.rl_bwt", tmp_path / "ids.txt", tmp_path / "bad.txt"
    img.write_bytes(b"\x01" + b"\0" * 7 + b"\x01" + b"\0" * 7 + b"\n\x01")
    ids.write_text("0 2\n5\t7\n")
    bad.write_text("0 2 x7 3\n")
    out = str(tmp_path / "out")
    text = os.path.join(GOLD, "test_byte_alphabet.txt")
    sel = ("--select", str(img))
    rc, _, err = run(cli, *sel, "--drop", str(ids))
    assert rc == 105 and "--output-file" in err                                   # --select without -o
    rc, _, err = run(cli, *sel, "--drop", str(ids), "-o", out, text)
    assert rc == 105 and "TEXT" in err                                            # with a TEXT argument
    rc, _, err = run(cli, *sel, "-o", out)
    assert rc == 105 and "--drop" in err and "--keep" in err                      # neither list
    rc, _, err = run(cli, *sel, "--drop", str(ids), "--keep", str(ids), "-o", out)
    assert rc == 105 and "--drop" in err and "--keep" in err                      # both
    rc, _, err = run(cli, *sel, "--drop", str(ids), "-o", out, "--gpus", "2")
    assert rc == 105 and "--gpus" in err
    rc, _, err = run(cli, *sel, "--keep", str(ids), "-o", out, "--fastx")
    assert rc == 105 and "--fastx" in err
    rc, _, err = run(cli, *sel, "--keep", str(ids), "-o", out, "-R")
    assert rc == 105 and "-R" in err
    rc, _, err = run(cli, "--select", str(tmp_path / "missing.rl_bwt"), "--drop", str(ids), "-o", out)
    assert rc == 105 and "--select" in err and "missing.rl_bwt" in err
    rc, _, err = run(cli, *sel, "--drop", str(tmp_path / "missing.txt"), "-o", out)
    assert rc == 105 and "--drop" in err and "missing.txt" in err
    rc, _, err = run(cli, *sel, "--keep", str(bad), "-o", out)
    assert rc == 105 and "--keep" in err and "x7" in err                          # a token that is no number
    rc, _, err = run(cli, *sel, "--drop", str(ids), "-o", out, "--sample-bits", "21")
    assert rc == 105 and "--sample-bits" in err
    assert run(cli, *sel, "--drop", str(ids), "-o", out, "-a", "3")[0] == 105
    assert run(cli, "--select")[0] == 114                                         # the image is missing
    rc, _, err = run(cli, "--drop", str(ids), text)
    assert rc == 105 and "--select" in err                                        # the lists belong to --select
    assert not os.path.exists(out + ".rl_bwt")
    rc, usage, _ = run(cli, "--help")
    assert rc == 0 and all(o in usage for o in ("--select", "--drop", "--keep", "--sample-bits"))


@pytest.mark.gpu
def test_cli_select_end_to_end(cli, tmp_path):
    rng = np.random.default_rng(31)
    a, b = mc.dna_pair(rng, 3000, 5200)
    ab = np.concatenate([a, b])
    ka, k = int((a == 10).sum()), int((ab == 10).sum())
    for name, cells in (("a", a), ("b", b), ("ab", ab)):
        (tmp_path / (name + ".txt")).write_bytes(cells.tobytes())
        rc, out, err = run(cli, str(tmp_path / (name + ".txt")), "-o", str(tmp_path / name))
        assert rc == 0, err
    (tmp_path / "ids.txt").write_text("\n".join(str(i) for i in range(ka, k)) + "\n")      # B's strings
    image = str(tmp_path / "ab.rl_bwt")
    rc, out, err = run(cli, "--select", image, "--drop", str(tmp_path / "ids.txt"), "-o", str(tmp_path / "dropped"))
    assert rc == 0, out[-2000:] + err[-2000:]
    assert (tmp_path / "dropped.rl_bwt").read_bytes() == (tmp_path / "a.rl_bwt").read_bytes()
    for label in ("Removing the listed strings", "Number of strings (in -> out)", "Number of symbols (in -> out)", "Strings listed", "Rows removed",
                  "Number of runs (in -> out)", "Bytes per run symbol", "Bytes per run length", "The resulting BCR BWT was stored in"):
        assert label in out, label
    rc, out, err = run(cli, "--select", image, "--keep", str(tmp_path / "ids.txt"), "-o", str(tmp_path / "kept"))
    assert rc == 0 and "Keeping the listed strings" in out, out[-2000:] + err[-2000:]
    assert (tmp_path / "kept.rl_bwt").read_bytes() == (tmp_path / "b.rl_bwt").read_bytes()
    rc, out, err = run(cli, "--select", image, "--drop", str(tmp_path / "ids.txt"), "--sample-bits", "4", "-o", str(tmp_path / "sampled"))
    assert rc == 0 and "Checkpoints" in out, out[-2000:] + err[-2000:]
    assert (tmp_path / "sampled.rl_bwt").read_bytes() == (tmp_path / "a.rl_bwt").read_bytes()
    # an id that is no string: a message and exit 2, no output file
    (tmp_path / "bad.txt").write_text("0 %d 1\n" % k)
    rc, out, err = run(cli, "--select", image, "--drop", str(tmp_path / "bad.txt"), "-o", str(tmp_path / "bad"))
    assert rc == 2 and "entry 1 " in err and not (tmp_path / "bad.rl_bwt").exists()
