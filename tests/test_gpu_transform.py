"""`poregen transform --signal FILE` on the MI355X: the two constants come from pa_stats' device path in the same process, so the model
equals, byte for byte, the one `--stdv S --mean M` gives for the `M<TAB>S` that `poregen pa_stats FILE` prints."""
import itertools
import os
import subprocess

import pytest

import bc_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "blow5", "example.blow5")


def run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=300)


def test_signal_equals_pa_stats_constants(tmp_path):
    names = ["".join(t) for t in itertools.product("ACGT", repeat=2)]
    raw = tmp_path / "raw_model"
    raw.write_text("".join(f"{k}\t{(i - 7) * 0.125 + 0.001953125}\t{1.5 + 0.1 * (i * 7 % 16):.1f}\n" for i, k in enumerate(names)))
    st = run("pa_stats", EXAMPLE)
    assert st.returncode == 0, st.stderr.decode()[-2000:]
    mean, stdv = st.stdout.decode().rstrip("\n").split("\t")
    assert bc_ref.is_number(mean) and bc_ref.is_number(stdv)
    want = run("transform", "--stdv", stdv, "--mean", mean, raw)
    assert want.returncode == 0, want.stderr.decode()[-2000:]
    assert want.stdout.decode() == bc_ref.transform(raw.read_text(), stdv, mean)
    got = run("transform", "--signal", EXAMPLE, "-o", tmp_path / "out.model", raw)
    assert got.returncode == 0 and got.stdout == b"", got.stderr.decode()[-2000:]
    assert (tmp_path / "out.model").read_bytes() == want.stdout
    assert f"[transform] --mean {mean} --stdv {stdv} ".encode() in got.stderr
