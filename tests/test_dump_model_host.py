"""`poregen model` without a device: the host path of a dump file (pg_dumphost.h: the pipeline's text tools restated) and the listing /
merging of dump directories (host/pg_dumpdir.h) against oracle/model_oracle.c, and the command's argument errors."""
import ctypes as C
import os
import subprocess
from decimal import Decimal

import pytest

from dump_cases import ODD_FILES, concatenated, regular_files_only, write_odd_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(os.environ.get("PG_ORACLE_DIR") or os.path.join(ROOT, "oracle"), "model_oracle")
BIN = os.path.join(ROOT, "bin", "poregen")


@pytest.fixture(scope="module")
def host():
    L = C.CDLL((os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so")))
    L.pgt_dump_model_host.argtypes = [C.POINTER(C.c_char_p), C.c_size_t, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.pgt_dump_model_host.restype = C.c_long
    L.pgt_model_texts.argtypes = [C.POINTER(C.c_longlong), C.c_size_t, C.c_char_p, C.c_char_p, C.c_size_t]
    return L


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    if not os.path.exists(ORACLE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])


def host_lines(L, dirs, which, limit="3.1", keep_first=0, threads=3):
    arr = (C.c_char_p * len(dirs))(*[os.fsencode(str(d)) for d in dirs])
    out = C.create_string_buffer(1 << 20); err = C.create_string_buffer(1024)
    n = L.pgt_dump_model_host(arr, len(dirs), which, limit.encode(), keep_first, threads, out, len(out), err, len(err))
    assert n >= 0, err.value.decode()
    return out.value.decode()


def oracle(mode, d, *args):
    return subprocess.run([ORACLE, mode, str(d)] + list(args), capture_output=True, check=True).stdout.decode()


def test_host_path_equals_the_oracle_on_the_odd_files(tmp_path, host):
    d = tmp_path / "odd"
    write_odd_dir(str(d))
    clean = regular_files_only(str(d), str(tmp_path / "clean"))
    for limit in ("3.1", "0.5"):
        assert host_lines(host, [d], 0, limit) == oracle("stats", clean, limit)
    assert host_lines(host, [d], 1) == oracle("dwell", clean)
    want = oracle("stats", clean, "3.1").splitlines()
    assert len(want) == len(ODD_FILES)                        # the dot file and the subdirectory are not listed
    by_name = {l.split("\t")[0]: l.split("\t")[1:] for l in want}
    assert by_name["AAAAA"] == ["", ""] and by_name["AAAAC"][0] == "2.5" and by_name["AAAGC"] == ["8.5", "nan"] and by_name["AAAGG"] == ["", ""]
    assert by_name["AAATC"][0] == "inf" and by_name["AAATA"] == ["20000001.5", "3.1"]


def test_strict_files_of_the_odd_directory_are_exact_on_the_device_path(tmp_path, host):
    """the device path prints the correctly rounded exact value (pg_model.h); on these files that is the oracle's text, so the GPU test
    may ask for equal lines"""
    d = tmp_path / "odd"
    write_odd_dir(str(d))
    want = {l.split("\t")[0]: l.rstrip("\n").split("\t")[1:] for l in oracle("stats", regular_files_only(str(d), str(tmp_path / "clean")), "1e9").splitlines()}
    for name, content, strict in ODD_FILES:
        if not strict:
            continue
        units = [int(Decimal(x).scaleb(8)) for x in content.replace(";", ",").split(",") if x][1:]
        med = C.create_string_buffer(64); sd = C.create_string_buffer(64)
        host.pgt_model_texts((C.c_longlong * len(units))(*units), len(units), med, sd, 64)
        assert [med.value.decode(), sd.value.decode()] == want[name], name


def test_two_directories_are_read_back_to_back(tmp_path, host):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    (a / "AAA").write_text("1.00000000,2.00000000;"); (b / "AAA").write_text("3.00000000,5.00000000;9.00000000;")   # tail drops 1.0 only
    (a / "AAC").write_text("1.50000000;")                                                                       # in a only
    (b / "AAG").write_text("4.00000000,4.50000000,8.00000000;")                                                 # in b only
    (a / "AAT").write_text("1.00000000,2.00000000"); (b / "AAT").write_text(".5,3.00000000;")                   # 2.00000000.5: not a number
    (a / "ACA").write_text("1.00000000,2.00000000;\n"); (b / "ACA").write_text("3.00000000;\n")                 # two awk records
    (b / ".AAA").write_text("7.00000000;")
    cat = concatenated([str(a), str(b)], str(tmp_path / "cat"))
    assert host_lines(host, [a, b], 0) == oracle("stats", cat, "3.1")
    assert host_lines(host, [a, b], 1) == oracle("dwell", cat)
    assert host_lines(host, [b, a], 0) == oracle("stats", concatenated([str(b), str(a)], str(tmp_path / "cat2")), "3.1")
    assert host_lines(host, [a, b], 0, keep_first=1).splitlines()[0] == "AAA\t3\t3.1"    # 1 2 3 5 9 with the first value kept
    assert [l.split("\t")[0] for l in host_lines(host, [a, b], 0).splitlines()] == ["AAA", "AAC", "AAG", "AAT", "ACA"]
    arr = (C.c_char_p * 1)(os.fsencode(str(tmp_path / "missing")))
    err = C.create_string_buffer(1024)
    assert host.pgt_dump_model_host(arr, 1, 0, b"3.1", 0, 1, None, 0, err, len(err)) == -1 and b"missing" in err.value


def test_model_usage_and_exit_codes(tmp_path):
    """argument errors only: they are settled before the device is asked for"""
    run = lambda *a: subprocess.run([BIN, "model"] + [str(x) for x in a], capture_output=True, text=True)
    r = run()
    assert r.returncode == 1 and "Usage: poregen model" in r.stderr
    r = run("--stdv_limit", "3.1")
    assert r.returncode == 1 and "Usage: poregen model" in r.stderr          # no directory
    r = run("-h")
    assert r.returncode == 0 and "Usage: poregen model" in r.stdout and "--dwell_model" in r.stdout
    d = tmp_path / "d"; d.mkdir(); (d / "AAAAA").write_text("1.00000000;")
    r = run("--stdv_limit", "abc", d)
    assert r.returncode == 1 and "--stdv_limit must be a number. You entered abc" in r.stderr
    r = run(d, tmp_path / "missing", "-o", tmp_path / "out")
    assert r.returncode == 1 and "missing" in r.stderr and not (tmp_path / "out").exists()
    r = run("--no_such_option", d)
    assert r.returncode == 1
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "model " in r.stdout
