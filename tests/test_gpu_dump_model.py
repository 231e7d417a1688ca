"""`poregen model` on the GPU: the k-mer model from the text of dump files (pg_dumptext.hip: device parser + the reduction of pg_model.hip)
against `gmove --raw_model` of the same run (byte for byte) and against oracle/model_oracle.c (tr | tail | datamash restated)."""
import os
import re
import subprocess
from decimal import Decimal

import numpy as np
import pytest

from dump_cases import ODD_FILES, concatenated, regular_files_only, write_odd_dir
from poregen_amd import synth
from poregen_amd.engine import DumpModel, model_from_dumps
from test_gpu_model import compare_raw_model, dump_from_oracle, exact_sstdev_text, oracle_lines  # noqa: F401  (dump_from_oracle: the oracle-made directories of that suite)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")


def run_model(dirs, out, dwell=None, limit=None, extra=(), env=None):
    """poregen model ... -> n_host_files as the command reports it"""
    cmd = [BIN, "model"] + [str(d) for d in dirs] + ["-o", str(out)] + list(extra)
    if dwell is not None:
        cmd += ["--dwell_model", str(dwell)]
    if limit is not None:
        cmd += ["--stdv_limit", limit]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    m = re.search(r"n_host_files: (\d+)", r.stderr)
    assert m, r.stderr
    return int(m.group(1))


def gmove_rna5(tmp_path, name, seed, extra=(), reads=300):
    """the synthetic k = 5 RNA set of test_cli_raw_model_and_dwell_model"""
    b = synth.make_batch(reads, kind="rna004", seed=seed)
    pre = str(tmp_path / (name + "_in"))
    synth.write_files(b, pre)
    out = tmp_path / name
    raw, dwell = tmp_path / (name + "_raw"), tmp_path / (name + "_dwell")
    r = subprocess.run([BIN, "gmove", "-k", "5", "--rna", "--scaling", "1", "--sample_limit", "50", "--min_dur", "19", "--max_dur", "51",
                        pre + ".slow5", pre + ".paf", str(out), "--fastq", pre + ".fastq", "--raw_model", str(raw), "--dwell_model", str(dwell),
                        "--stdv_limit", "0.9"] + (list(extra) if extra else ["--file_limit", "1024"]), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    return out, raw, dwell


def test_round_trip_equals_gmove_raw_model(tmp_path):
    out, raw, dwell = gmove_rna5(tmp_path, "out", 31)
    a2, b2 = tmp_path / "A2", tmp_path / "B2"
    n_host = run_model([out / "dump"], a2, b2, "0.9")
    assert a2.read_bytes() == raw.read_bytes() and b2.read_bytes() == dwell.read_bytes()
    assert n_host == 0
    assert "\t0.9\n" in a2.read_text()
    # the same in several small batches
    a3, b3 = tmp_path / "A3", tmp_path / "B3"
    assert run_model([out / "dump"], a3, b3, "0.9", extra=["-t", "3"], env=dict(os.environ, POREGEN_MODEL_BATCH="20000")) == 0
    assert a3.read_bytes() == raw.read_bytes() and b3.read_bytes() == dwell.read_bytes()
    # --keep_first: one more value in every file that has any
    a4 = tmp_path / "A4"
    run_model([out / "dump"], a4, extra=["--keep_first"])
    assert a4.read_bytes() != a2.read_bytes()


def test_against_the_oracle(tmp_path):
    out, _, _ = gmove_rna5(tmp_path, "out", 31)
    d = out / "dump"
    want_dwell = "".join(oracle_lines(d, "dwell"))
    for limit in ("3.1", "0.5"):
        a, b = tmp_path / ("A" + limit), tmp_path / ("B" + limit)
        assert run_model([d], a, b, limit) == 0
        compare_raw_model(a.read_text(), oracle_lines(d, "stats", limit), d, limit)
        assert b.read_text() == want_dwell
        raw_lines, dwell_lines, info = model_from_dumps([d], limit=limit)
        assert raw_lines == a.read_text() and dwell_lines == want_dwell
        assert info.n_host_files == 0 and info.n_files == 1024 and info.n_bytes == sum(os.path.getsize(d / n) for n in os.listdir(d))
    raw_lines, _, info = model_from_dumps(d, batch_bytes=30000)                   # several submissions
    assert raw_lines == (tmp_path / "A3.1").read_text() and info.n_batches > 3


def test_several_directories(tmp_path):
    o1, _, _ = gmove_rna5(tmp_path, "o1", 31, extra=["--index_start", "1", "--index_end", "600"])
    o2, _, _ = gmove_rna5(tmp_path, "o2", 32, extra=["--index_start", "400", "--index_end", "1024"])
    d1, d2 = o1 / "dump", o2 / "dump"
    assert len(os.listdir(d1)) == 600 and len(os.listdir(d2)) == 625
    for dirs, name in (([d1, d2], "cat12"), ([d2, d1], "cat21")):
        cat = concatenated([str(x) for x in dirs], str(tmp_path / name))
        a, b = tmp_path / ("A" + name), tmp_path / ("B" + name)
        assert run_model(dirs, a, b, "3.1") == 0
        assert len(a.read_text().splitlines()) == 1024
        compare_raw_model(a.read_text(), oracle_lines(cat, "stats", "3.1"), cat, "3.1")
        assert b.read_text() == "".join(oracle_lines(cat, "dwell"))
    assert (tmp_path / "Acat12").read_text() != (tmp_path / "Acat21").read_text()   # tail drops another first value


def test_odd_files(tmp_path):
    d = tmp_path / "odd"
    n_strict, n_outside = write_odd_dir(str(d))
    clean = regular_files_only(str(d), str(tmp_path / "clean"))
    for limit in ("3.1", "0.5"):
        a, b = tmp_path / ("A" + limit), tmp_path / ("B" + limit)
        n_host = run_model([d], a, b, limit)
        assert a.read_text() == "".join(oracle_lines(clean, "stats", limit))
        assert b.read_text() == "".join(oracle_lines(clean, "dwell"))
        assert n_host == n_outside and n_strict + n_outside == len(ODD_FILES)
        raw_lines, dwell_lines, info = model_from_dumps([d], limit=limit)
        assert raw_lines == a.read_text() and dwell_lines == b.read_text() and info.n_host_files == n_outside
        assert [ODD_FILES[i][0] for i in info.host_files] == [f[0] for f in ODD_FILES if not f[2]]


def test_negative_zero_median_is_finished_on_the_host(tmp_path):
    """datamash prints the sign of a median of -0; the integers of the device path have none, so such a file takes the host path"""
    d = tmp_path / "z"
    d.mkdir()
    (d / "AAAAA").write_text("1.00000000,-0.00000000;")                                  # the median is -0
    (d / "AAAAC").write_text("1.00000000,-0.00000000,0.00000000,-0.00000000;")           # +-0 among themselves: the oracle's sort decides
    (d / "AAAAG").write_text("1.00000000,-0.00000000,2.00000000,-2.00000000;")           # the median is -0 too, with other values around
    (d / "AAAAT").write_text("1.00000000,-0.00000000,2.00000000,3.00000000;")            # a negative zero, median 2: device
    raw_lines, dwell_lines, info = model_from_dumps([d])
    assert raw_lines == "".join(oracle_lines(d, "stats", "3.1")) and dwell_lines == "".join(oracle_lines(d, "dwell"))
    assert "AAAAA\t-0\t" in raw_lines
    assert list(info.host_files) == [0, 1, 2]


def _write_values(path, units, rng):
    """units (integers of 1e-8) as gmove prints them, in events of 3 to 11 values"""
    out, i = [], 0
    while i < len(units):
        n = int(rng.integers(3, 12))
        ev = units[i:i + n]
        out.append(",".join("%s%d.%08d" % ("-" if u < 0 else "", abs(u) // 10**8, abs(u) % 10**8) for u in ev) + ";")
        i += n
    with open(path, "w") as f:
        f.write("".join(out))


def test_every_kernel_class(tmp_path):
    """files of 1 000, 2 000, 4 000 and 20 000 values: the one-wave, 32-row, 256-thread and 1024-thread kernels of pg_model.hip fed with
    parsed units; against the oracle's text and against Python integers"""
    rng = np.random.default_rng(20261017)
    d = tmp_path / "kinds"
    d.mkdir()
    names = ["AAAAA", "AAAAC", "AAAAG", "AAAAT", "AAACA", "AAACC"]
    sizes = [1000, 2000, 4000, 20000, 1025, 4097]
    scale = [1.5e8, 2.0e10, 1.0e8, 9.0e9, 3.9e15 / 4, 1.0e6]      # also 8-digit integer parts and a spread in the low digits only
    files = []
    for name, n, sc in zip(names, sizes, scale):
        u = [int(x) for x in np.clip(rng.normal(0.0, 1.0, n), -3.5, 3.5) * sc]
        if name == "AAACA":
            u = [3_999_999_999_999_999 - abs(x) % (1 << 39) for x in u]      # next to the largest value, inside the moment sums' spread
        files.append(u)
        _write_values(d / name, u, rng)
    assert any(x < 0 for x in files[0])
    raw_lines, dwell_lines, info = model_from_dumps([d], limit="1e9")
    assert info.n_host_files == 0 and info.n_values == sum(sizes)
    want = oracle_lines(d, "stats", "1e9")
    got = raw_lines.splitlines(keepends=True)
    for name, g, w in zip(names, got, want):
        if name == "AAACA":    # values of 4e7: strtold's long double is 3.6e-12 off each of them, and the oracle's texts with it
            gk, gm, gs = g.rstrip("\n").split("\t"); wk, wm, ws = w.rstrip("\n").split("\t")
            assert gk == wk and abs(Decimal(gm) - Decimal(wm)) <= Decimal("1e-6"), (g, w)          # the median: one unit of its 14th digit
            exact = exact_sstdev_text(os.path.join(str(d), gk))
            assert abs(Decimal(gs) - exact) <= Decimal(1).scaleb(exact.adjusted() - 13) / 2, (g, exact)   # the device text: the exact value, rounded
            assert abs(Decimal(ws) - exact) <= abs(exact) * Decimal("1e-9"), (w, exact)
        else:
            compare_raw_model(g, [w], str(d), "1e9")
    assert dwell_lines == "".join(oracle_lines(d, "dwell"))
    dm = DumpModel(keep_first=True)
    blob = b"".join(open(d / n, "rb").read() for n in names)
    off = np.cumsum([0] + [os.path.getsize(d / n) for n in names])
    import torch
    for data in (blob, torch.frombuffer(bytearray(b"x" + blob), dtype=torch.uint8).cuda()[1:]):    # host bytes; device bytes, unaligned
        dm.submit(data, off)
        m, info = dm.finish()
        assert info.n_host_files == 0
        for s, u in enumerate(files):
            su = sorted(u); n = len(u)
            assert int(m.n_values[s]) == n and (int(m.mid_lo[s]), int(m.mid_hi[s])) == (su[(n - 1) // 2], su[n // 2]), s
            dd = [x - u[0] for x in u]
            assert int(m.origin[s]) == u[0] and int(m.sum1[s]) == sum(dd), s
            assert (int(m.sum2_hi[s]) << 64) + int(m.sum2_lo[s]) == sum(x * x for x in dd), s
    dm.close()


def test_k9_layout(tmp_path):
    """262 144 files, most of them empty: every line of `poregen model` equals `gmove --raw_model` of the run that wrote them"""
    b = synth.make_batch(400, kind="dna_r10", seed=99)
    pre = str(tmp_path / "in")
    synth.write_files(b, pre)
    out = tmp_path / "out"
    raw, dwell = tmp_path / "raw", tmp_path / "dwell"
    r = subprocess.run([BIN, "gmove", "-k", "9", "--file_limit", "262144", "--sample_limit", "3", pre + ".slow5", pre + ".paf", str(out),
                        "--fastq", pre + ".fastq", "--raw_model", str(raw), "--dwell_model", str(dwell)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    a2, b2 = tmp_path / "A2", tmp_path / "B2"
    n_host = run_model([out / "dump"], a2, b2)
    got, want = a2.read_text().splitlines(), raw.read_text().splitlines()
    assert len(got) == 262144 == len(want)
    assert got == want and b2.read_bytes() == dwell.read_bytes()
    assert n_host == 0
    assert sum(1 for l in got if not l.endswith("\t\t")) > 100
