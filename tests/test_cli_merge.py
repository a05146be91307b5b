"""`grlbwt --merge A.rl_bwt B.rl_bwt -o OUT`: the argument contract (no GPU), and the merged file against the file the command
line builds from the concatenated text."""
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


def test_cli_merge_argument_contract(cli, tmp_path):
    a, b = tmp_path / "a.rl_bwt", tmp_path / "b.rl_bwt"
    a.write_bytes(b"\x01" + b"\0" * 7 + b"\x01" + b"\0" * 7 + b"\n\x01")
    b.write_bytes(a.read_bytes())
    out = str(tmp_path / "out")
    text = os.path.join(GOLD, "test_byte_alphabet.txt")
    rc, _, err = run(cli, "--merge", str(a), str(b))
    assert rc == 105 and "--output-file" in err                                   # --merge without -o
    rc, _, err = run(cli, "--merge", str(a), str(b), "-o", out, text)
    assert rc == 105 and "TEXT" in err                                            # with a TEXT argument
    rc, _, err = run(cli, "--merge", str(a), str(b), "-o", out, "--gpus", "2")
    assert rc == 105 and "--gpus" in err
    assert run(cli, "--merge", str(a), str(b), "-o", out, "--fastx")[0] == 105
    assert run(cli, "--merge", str(a), str(b), "-o", out, "-R")[0] == 105
    assert run(cli, "--merge", str(a), str(tmp_path / "missing.rl_bwt"), "-o", out)[0] == 105
    assert run(cli, "--merge", str(a), str(b), "-o", out, "-a", "3")[0] == 105
    assert run(cli, "--merge", str(a))[0] == 114                                  # the second image is missing
    assert not os.path.exists(out + ".rl_bwt")
    rc, usage, _ = run(cli, "--help")
    assert rc == 0 and "--merge" in usage


@pytest.mark.gpu
def test_cli_merge_end_to_end(cli, tmp_path):
    rng = np.random.default_rng(31)
    a, b = mc.dna_pair(rng, 3000, 5200)
    for name, cells in (("a", a), ("b", b), ("ab", np.concatenate([a, b]))):
        (tmp_path / (name + ".txt")).write_bytes(cells.tobytes())
        rc, out, err = run(cli, str(tmp_path / (name + ".txt")), "-o", str(tmp_path / name))
        assert rc == 0, err
    rc, out, err = run(cli, "--merge", str(tmp_path / "a.rl_bwt"), str(tmp_path / "b.rl_bwt"), "-o", str(tmp_path / "merged"))
    assert rc == 0, out[-2000:] + err[-2000:]
    assert (tmp_path / "merged.rl_bwt").read_bytes() == (tmp_path / "ab.rl_bwt").read_bytes()
    for label in ("Merging the BWTs", "Number of strings (A + B)", "Refinement rounds", "Number of runs (r)", "The resulting BCR BWT was stored in"):
        assert label in out, label
    # images of different separators: a message and exit 2, no output file
    (tmp_path / "z.txt").write_bytes(np.where(b == 10, 0, b).astype(np.uint8).tobytes())
    assert run(cli, str(tmp_path / "z.txt"), "-o", str(tmp_path / "z"))[0] == 0
    rc, out, err = run(cli, "--merge", str(tmp_path / "a.rl_bwt"), str(tmp_path / "z.rl_bwt"), "-o", str(tmp_path / "bad"))
    assert rc == 2 and "smallest symbols" in err and not (tmp_path / "bad.rl_bwt").exists()
