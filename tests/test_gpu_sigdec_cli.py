"""`poregen subtool0` / `pa_stats` on files with svb-zd signals, which the device decodes: the same bytes as for the same reads stored
uncompressed, whatever the record compression; the reference's golden file; and a block only the device can refuse ends the run as
the host decoder's refusal did."""
import os
import re
import subprocess

import numpy as np
import pytest

import pamean_ref as R
import sigdec_cases as K
import sigdec_ref as S
from poregen_amd import synth
from test_gpu_pamean import records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
B5 = os.path.join(ROOT, "tests", "golden", "blow5")


def run(*args, cmd="subtool0", env=None):
    return subprocess.run([BIN, cmd] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **(env or {})), timeout=600)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("svb")
    recs = [x for x in records(seed=6, with_long=True) if x[2] != 0.0 and x[4] != 0.0]
    out = {}
    for kind in ("none", "none+svb-zd", "zlib+svb-zd", "zstd+svb-zd"):
        rp, _, sp = kind.partition("+")
        if rp == "zstd" and synth.zstd_compress(b"x") is None:
            continue
        out[kind] = d / (kind.replace("+", "_") + ".blow5")
        R.write_blow5(out[kind], recs, rp, sp or "none")
    return recs, out


@pytest.mark.parametrize("cmd", ["subtool0", "pa_stats"])
@pytest.mark.parametrize("kind", ["none+svb-zd", "zlib+svb-zd", "zstd+svb-zd"])
def test_same_bytes_as_the_uncompressed_file(files, cmd, kind):
    recs, paths = files
    if kind not in paths:
        pytest.skip("no libzstd.so.1 on this machine")
    want = run(paths["none"], cmd=cmd)
    assert want.returncode == 0 and want.stdout and (cmd != "subtool0" or want.stdout == R.lines(recs))
    for env in (None, {"POREGEN_PAMEAN_BATCH_BYTES": "20000"}):
        r = run(paths[kind], cmd=cmd, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == want.stdout, (kind, env)


def test_the_blocks_are_decoded_on_the_device(files):
    """-v 4 adds the count of pg_pamean_svb_samples to the summary on stderr: every sample of an svb-zd file, none of a raw one"""
    recs, paths = files
    total = sum(len(r[1]) for r in recs)
    for kind, path in paths.items():
        r = run("-v", 4, path)
        assert r.returncode == 0 and r.stdout == R.lines(recs)
        m = re.search(rb"\[subtool0\] (\d+) samples decoded from svb-zd blocks on the device", r.stderr)
        assert m and int(m.group(1)) == (0 if kind == "none" else total), (kind, r.stderr)
    assert b"decoded from svb-zd" not in run(paths["zlib+svb-zd"]).stderr       # the default summary is what it was


def test_reference_golden_example():
    r = run(os.path.join(B5, "example.blow5"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == open(os.path.join(B5, "example.exp"), "rb").read()


@pytest.mark.parametrize("press", ["none", "zlib"])
def test_a_block_only_the_device_can_refuse_ends_the_run_like_the_host_decoder(tmp_path, press):
    """record 5's block passes every check the host makes; its byte lengths run past its data. One record per batch: the records in
    front of the batch before the bad one's are printed, then the host decoder's message and exit status 1."""
    rng = np.random.default_rng(2)
    recs = [(f"r{i}", S.encode(rng.normal(500, 60, 50 + i).astype(np.int16)), 2048.0, -240.0, 281.0) for i in range(8)]
    zz, nb = K.case("alternating", 300, rng)
    recs[5] = ("r5", S.encode_values(zz, nb)[:-3], 2048.0, -240.0, 281.0)
    p = tmp_path / "x.blow5"
    S.write_blow5_blocks(p, recs, press)
    good = [(rid, S.decode(blk), d, o, r) for rid, blk, d, o, r in recs[:5]]
    for env, n_printed in (({"POREGEN_PAMEAN_BATCH_BYTES": "1"}, 4), (None, 0)):
        r = run(p, env=env)
        assert r.returncode == 1
        assert r.stdout == R.lines(good[:n_printed]), env
        assert re.search(rb"\[subtool0::ERROR\].*Error parsing the record: record 5: corrupt streamvbyte block", r.stderr), r.stderr
