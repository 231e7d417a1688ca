"""`poregen simulate --compress / --sig_compress`: one small run written five ways. The compressed files hold the default file's samples,
every other output is the default run's byte for byte, the readers of the project (subtool0, gmove) make of each file what they make of
the default one, and the file's bytes depend neither on -t nor on --batch_reads."""
import ctypes as C
import filecmp
import os
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import sigenc_cases as EK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
K3 = 3
WAYS = {"default": [], "svb": ["--sig_compress", "svb-zd"], "zlib_svb": ["--compress", "zlib", "--sig_compress", "svb-zd"], "zlib": ["--compress", "zlib"],
        "zstd_svb": ["--compress", "zstd", "--sig_compress", "svb-zd"]}
HEAD = {"default": (0, 0), "svb": (0, 1), "zlib_svb": (1, 1), "zlib": (1, 0), "zstd_svb": (2, 1)}


def run(*args):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def kmers(k):
    out = [""]
    for _ in range(k):
        out = [p + c for p in out for c in "ACGT"]
    return out


def shim():
    h = K.hosttest()
    h.pgt_slow5_get.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]; h.pgt_slow5_get.restype = C.c_long
    h.pgt_slow5_walk.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]; h.pgt_slow5_walk.restype = C.c_long
    h.pgt_zstd_can_compress.restype = C.c_int
    return h


def file_reads(h, path):
    """[(id, samples, calibration)] in file order, through the project's reader"""
    ids, lens, err = C.create_string_buffer(1 << 16), np.zeros(4096, np.uint64), C.create_string_buffer(512)
    n = h.pgt_slow5_walk(str(path).encode(), ids, len(ids), lens.ctypes.data, lens.size, err, len(err))
    assert n >= 0, err.value
    out = []
    for rid, ln in zip(ids.value.decode().split("\n")[:n], lens[:n]):
        cal, raw = np.zeros(3), np.zeros(max(int(ln), 1), np.int16)
        assert h.pgt_slow5_get(str(path).encode(), rid.encode(), cal.ctypes.data, raw.ctypes.data, int(ln)) == int(ln), rid
        out.append((rid, raw[:int(ln)].copy(), tuple(cal)))
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """70 contigs of 20 to 60 bases, one of 600 (more than a piece of 4 096 samples at 10 samples a base) and one of 2 bases, which the
    generator refuses; --full_contigs makes a read of each. Every way of writing runs once."""
    d = tmp_path_factory.mktemp("sigenc_cli")
    rng = np.random.default_rng(99)
    levels, stdvs = (60000 + 900 * rng.permutation(64)).astype(int), rng.integers(1500, 3000, 64).astype(int)
    model = d / "k3.model"
    model.write_text("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{levels[i] / 1000:.3f}\t{stdvs[i] / 1000:.3f}\n" for i, km in enumerate(kmers(K3))))
    seq = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    contigs = [(f"c{i}", seq(int(n))) for i, n in enumerate(rng.integers(20, 61, 70))]
    contigs.insert(10, ("long", seq(600)))
    contigs.insert(40, ("tiny", seq(2)))
    ref = d / "ref.fa"
    ref.write_text("".join(f">{n}\n{s}\n" for n, s in contigs))
    h = shim()
    zstd = bool(h.pgt_zstd_can_compress())
    common = ["-k", K3, "--seed", 12, "--full_contigs", "--lead", 7, model, ref]
    for way, opts in WAYS.items():
        rc, _, err = run("simulate", "-o", d / f"{way}.blow5", "-c", d / f"{way}.paf", "-q", d / f"{way}.fastq", "--moves", d / f"{way}.sam", *opts, *common)
        if way == "zstd_svb" and not zstd:
            assert rc == 1 and "libzstd.so.1" in err and not (d / f"{way}.blow5").exists()
            continue
        assert rc == 0 and f"reads={len(contigs)} written={len(contigs) - 1} refused=1" in err, (way, err)
    return dict(dir=d, model=model, ref=ref, common=common, h=h, ways=[w for w in WAYS if w != "zstd_svb" or zstd], n=len(contigs) - 1)


def test_the_other_outputs_do_not_change(world):
    d = world["dir"]
    for way in world["ways"]:
        for ext in ("paf", "fastq", "sam"):
            assert (d / f"{way}.{ext}").read_bytes() == (d / f"default.{ext}").read_bytes(), (way, ext)
    assert (d / "default.paf").read_bytes().count(b"\n") == world["n"]


def test_every_file_holds_the_default_files_samples(world):
    d, h = world["dir"], world["h"]
    want = file_reads(h, d / "default.blow5")
    assert len(want) == world["n"] and max(r[1].size for r in want) > EK.V_PIECE and "tiny" not in [r[0] for r in want]
    sizes = {}
    for way in world["ways"]:
        b = (d / f"{way}.blow5").read_bytes()
        assert (b[9], b[14]) == HEAD[way], way
        sizes[way] = len(b)
        got = file_reads(h, d / f"{way}.blow5")
        assert [g[0] for g in got] == [w[0] for w in want] and all(np.array_equal(g[1], w[1]) and g[2] == w[2] for g, w in zip(got, want)), way
    print("file bytes:", sizes)
    assert sizes["svb"] < sizes["default"]


def test_subtool0_prints_the_same_lines(world):
    d = world["dir"]
    out = {}
    for way in world["ways"]:
        r = subprocess.run([BIN, "subtool0", str(d / f"{way}.blow5")], capture_output=True, timeout=120)
        assert r.returncode == 0, (way, r.stderr)
        out[way] = r.stdout
    assert out["default"].count(b"\n") >= world["n"] and all(o == out["default"] for o in out.values())


def test_the_file_does_not_depend_on_threads_or_batches(world):
    d = world["dir"]
    for name, opts in (("t1", ["-t", 1]), ("t4", ["-t", 4]), ("b7", ["--batch_reads", 7])):
        rc, _, err = run("simulate", "-o", d / f"{name}.blow5", *WAYS["zlib_svb"], *opts, *world["common"])
        assert rc == 0, err
        assert (d / f"{name}.blow5").read_bytes() == (d / "zlib_svb.blow5").read_bytes(), name
    rc, _, err = run("simulate", "-o", d / "b7raw.blow5", "--batch_reads", 7, *WAYS["zlib"], *world["common"])
    assert rc == 0 and (d / "b7raw.blow5").read_bytes() == (d / "zlib.blow5").read_bytes(), err


def test_gmove_collects_the_same_dump(world):
    d = world["dir"]
    for way in ("default", "zlib_svb"):
        rc, _, err = run("gmove", "-k", K3, "--scaling", 0, d / f"{way}.blow5", d / f"{way}.paf", d / f"out_{way}", "--fastq", d / f"{way}.fastq")
        assert rc == 0, err
    a, b = d / "out_default" / "dump", d / "out_zlib_svb" / "dump"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) >= 64
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors and sum(os.path.getsize(a / n) for n in names) > 0


def test_refusals(world):
    d = world["dir"]
    rc, _, err = run("simulate", "-o", d / "no.slow5", "--sig_compress", "svb-zd", *world["common"])
    assert rc == 1 and "are for a .blow5 file" in err and not (d / "no.slow5").exists()
    rc, _, err = run("simulate", "-o", d / "no.blow5", "--compress", "gzip", *world["common"])
    assert rc == 1 and "is not a value it takes" in err and not (d / "no.blow5").exists()
