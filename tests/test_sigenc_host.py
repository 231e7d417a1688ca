"""The svb-zd encoder's rule and the BLOW5 writer that takes its blocks, without a GPU (through _pg_hosttest.so): the host statement of
the rule (csrc/pg_svb.h: pg_svb_encode_host) against tests/sigdec_ref.py: encode(), the bound, the blocks slow5tools wrote into
tests/golden/blow5/example.blow5, the writer's compressed forms read back by the project's reader, and the command's argument errors."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import sigdec_ref as S
import sigenc_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "blow5", "example.blow5")


@pytest.fixture(scope="module")
def shim():
    h = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    h.pgt_svb_bound.argtypes = [C.c_uint64]; h.pgt_svb_bound.restype = C.c_uint64
    h.pgt_svb_max_v.restype = C.c_uint32
    h.pgt_svb_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]; h.pgt_svb_encode.restype = C.c_uint64
    h.pgt_sim_write_blow5.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_uint, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_char_p, C.c_size_t]
    h.pgt_slow5_walk.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]; h.pgt_slow5_walk.restype = C.c_long
    h.pgt_slow5_svb_walk.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]; h.pgt_slow5_svb_walk.restype = C.c_long
    h.pgt_slow5_get.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]; h.pgt_slow5_get.restype = C.c_long
    return h


def host_encode(shim, s):
    s = np.ascontiguousarray(s, np.int16)
    cap = 4 + (s.size + 3) // 4 + 3 * s.size
    out = np.full(cap + 8, 0xAA, np.uint8)
    n = shim.pgt_svb_encode(s.ctypes.data if s.size else None, s.size, out.ctypes.data, cap)
    assert n <= cap and (out[cap:] == 0xAA).all()
    return out[:n].tobytes()


def test_rule_equals_the_reference_and_decodes_back(shim):
    rng = np.random.default_rng(11)
    small = [rng.integers(-32768, 32768, int(n)).astype(np.int16) if i % 2 else K.walk(rng, int(n)) for i, n in enumerate(rng.integers(0, 70, 200))]
    for name, s in [(n, s) for n, s in K.reads() if not n.startswith("short_")] + [(f"random_{i}", s) for i, s in enumerate(small)]:
        got = host_encode(shim, s)
        assert got == S.encode(s), name
        back = S.decode(got)
        assert back is not None and np.array_equal(back, s), name


def test_bound(shim):
    """4 + ceil(n / 4) + 3 n bounds every block. No read reaches it: |s_0 - 0| <= 32 768 gives a zig-zag value below 2^16, so the first
    value never takes 3 bytes. The longest block there is, one byte below the bound, belongs to the read that alternates between
    +-32 767 (every later |delta| is 65 534), and among the cases of two samples or more to no other read (a read of one sample gets
    there with any 2-byte value)."""
    assert shim.pgt_svb_max_v() == 131070 == int(S.zigzag(np.array([-32768, 32767], np.int16)).max())
    for n in (0, 1, 2, 3, 4, 5, 255, 4096, 2 ** 32 - 1):
        assert shim.pgt_svb_bound(n) == 4 + (n + 3) // 4 + 3 * n
    assert len(host_encode(shim, np.zeros(0, np.int16))) == 4 == shim.pgt_svb_bound(0)
    near = set()
    for name, s in K.reads():
        if s.size:
            got = len(host_encode(shim, s))
            assert got <= shim.pgt_svb_bound(s.size) - 1, name
            if s.size >= 2 and got == shim.pgt_svb_bound(s.size) - 1:
                near.add(name)
    assert near == {"all_3_byte", "all_3_byte_neg"}
    for n in (1, 2, 7, 4097):
        assert len(host_encode(shim, K.alternating(n, 32767))) == shim.pgt_svb_bound(n) - 1


def walk_ids(shim, path):
    ids, lens, err = C.create_string_buffer(1 << 16), np.zeros(4096, np.uint64), C.create_string_buffer(512)
    n = shim.pgt_slow5_walk(str(path).encode(), ids, len(ids), lens.ctypes.data, lens.size, err, len(err))
    assert n >= 0, err.value
    return ids.value.decode().split("\n")[:n], [int(x) for x in lens[:n]]


def svb_walk(shim, path):
    cap = 1 << 22
    counts, lens, blocks, err = np.zeros(4096, np.uint32), np.zeros(4096, np.uint64), np.zeros(cap, np.uint8), C.create_string_buffer(512)
    n = shim.pgt_slow5_svb_walk(str(path).encode(), counts.ctypes.data, lens.ctypes.data, 4096, blocks.ctypes.data, cap, err, 512)
    assert n >= 0, err.value
    off = np.concatenate([[0], np.cumsum(lens[:n])]).astype(np.int64)
    assert int(off[-1]) <= cap
    return [int(c) for c in counts[:n]], [blocks[off[i]:off[i + 1]].tobytes() for i in range(n)]


def get_read(shim, path, rid, n):
    cal, raw = np.zeros(3), np.zeros(max(n, 1), np.int16)
    assert shim.pgt_slow5_get(str(path).encode(), rid.encode(), cal.ctypes.data, raw.ctypes.data, n) == n, rid
    return raw[:n].copy(), tuple(cal)


def test_golden_blocks_of_slow5tools(shim):
    """example.blow5 (zlib records, svb-zd signals, written by slow5tools): every read decoded by the project's reader and encoded again
    is the file's own block, byte for byte."""
    ids, lens = walk_ids(shim, EXAMPLE)
    counts, blocks = svb_walk(shim, EXAMPLE)
    assert len(ids) == 5 and counts == lens and sum(lens) == 298365 and max(lens) == 59676
    for rid, n, blk in zip(ids, lens, blocks):
        raw, _ = get_read(shim, EXAMPLE, rid, n)
        assert host_encode(shim, raw) == blk == S.encode(raw), rid


def blow5_records(path):
    """(header bytes 9 and 14, [record bytes as they lie in the file])"""
    b = open(path, "rb").read()
    assert b[:6] == b"BLOW5\x01" and b[-5:] == b"5WOLB"
    pos = 68 + struct.unpack_from("<I", b, 64)[0]
    recs = []
    while pos < len(b) - 5:
        sz = struct.unpack_from("<Q", b, pos)[0]
        recs.append(b[pos + 8:pos + 8 + sz])
        pos += 8 + sz
    assert pos == len(b) - 5
    return b[9], b[14], recs


def body(rid, d, o, r, len_field, payload):
    rid = rid.encode()
    return struct.pack("<H", len(rid)) + rid + struct.pack("<I", 0) + struct.pack("<dddd", d, o, r, 4000.0) + struct.pack("<Q", len_field) + payload


WRITER_READS = ("len_0", "len_1", "len_5", "len_257", "len_4097", "all_3_byte", "first_low")


def write(shim, path, rec, sig, threads=2, binary=1):
    rs = [s for n, s in K.reads() if n in WRITER_READS]
    ids = b"".join(f"read_{i}".encode() + b"\0" for i in range(len(rs)))
    n = len(rs)
    dig, ofs, rg = np.full(n, 8192.0), np.arange(n, dtype=np.float64) - 3, np.full(n, 1467.61)
    parts = [S.encode(s) if sig == "svb-zd" else s.tobytes() for s in rs]
    unit = 1 if sig == "svb-zd" else 2
    off = np.zeros(n + 1, np.uint64); off[1:] = np.cumsum([len(p) // unit for p in parts])
    data = np.frombuffer(b"".join(parts) + b"\0", np.uint8)
    err = C.create_string_buffer(512)
    rc = shim.pgt_sim_write_blow5(str(path).encode(), binary, rec.encode(), sig.encode(), threads, n, ids, dig.ctypes.data, ofs.ctypes.data, rg.ctypes.data, data.ctypes.data,
                                  off.ctypes.data, err, 512)
    return rc, err.value.decode(), rs, parts, (dig, ofs, rg)


@pytest.mark.parametrize("rec,sig", [("none", "svb-zd"), ("zlib", "svb-zd"), ("zlib", "none"), ("zstd", "svb-zd"), ("zstd", "none"), ("none", "none")])
def test_writer_forms_read_back(shim, tmp_path, rec, sig):
    if rec == "zstd" and not shim.pgt_zstd_can_compress():
        rc, err, *_ = write(shim, tmp_path / "z.blow5", rec, sig)
        assert rc == -1 and "libzstd.so.1" in err and not (tmp_path / "z.blow5").exists()   # refused before the file is opened
        return
    path = tmp_path / f"{rec}_{sig}.blow5"
    rc, err, rs, parts, (dig, ofs, rg) = write(shim, path, rec, sig)
    assert rc == 0, err
    b9, b14, recs = blow5_records(path)
    assert b9 == {"none": 0, "zlib": 1, "zstd": 2}[rec] and b14 == {"none": 0, "svb-zd": 1}[sig] and len(recs) == len(rs)
    want = [body(f"read_{i}", dig[i], ofs[i], rg[i], len(p) if sig == "svb-zd" else s.size, p) for i, (s, p) in enumerate(zip(rs, parts))]
    if rec == "zlib":
        assert [zlib.decompress(r) for r in recs] == want                                   # one whole zlib stream per record
    elif rec == "none":
        assert recs == want
    ids, lens = walk_ids(shim, path)
    assert ids == [f"read_{i}" for i in range(len(rs))] and lens == [s.size for s in rs]
    for i, s in enumerate(rs):
        raw, cal = get_read(shim, path, f"read_{i}", s.size)
        assert np.array_equal(raw, s) and cal == (dig[i], ofs[i], rg[i])
    if sig == "svb-zd":
        counts, blocks = svb_walk(shim, path)
        assert counts == [s.size for s in rs] and blocks == parts
    for threads in (1, 5):                                                                  # the file does not depend on the threads
        other = tmp_path / f"t{threads}.blow5"
        assert write(shim, other, rec, sig, threads=threads)[0] == 0 and other.read_bytes() == path.read_bytes()


def test_writer_refusals(shim, tmp_path):
    for rec, sig in (("zlib", "none"), ("none", "svb-zd")):
        rc, err, *_ = write(shim, tmp_path / "a.slow5", rec, sig, binary=0)
        assert rc == -1 and "ASCII" in err and not (tmp_path / "a.slow5").exists()
    assert write(shim, tmp_path / "b.blow5", "gzip", "none")[0] == -2 and write(shim, tmp_path / "b.blow5", "none", "svb")[0] == -2


def simulate(args):
    return subprocess.run([BIN, "simulate"] + [str(a) for a in args], capture_output=True, text=True)


def test_command_argument_errors(tmp_path):
    """Refused while the arguments are read: nothing is opened, no device is asked for."""
    model, ref = tmp_path / "none.model", tmp_path / "none.fa"
    for bad in (["--compress", "gzip"], ["--compress", ""], ["--sig_compress", "svb"], ["--sig_compress", "ex-zd"], ["-t", "0"], ["-t", "x"]):
        r = simulate(bad + ["-o", tmp_path / "a.blow5", model, ref])
        assert r.returncode == 1 and "is not a value it takes" in r.stderr, bad
    for bad in (["--sig_compress", "svb-zd"], ["--compress", "zlib"], ["--compress", "zstd", "--sig_compress", "svb-zd"]):
        r = simulate(bad + ["-o", tmp_path / "a.slow5", model, ref])
        assert r.returncode == 1 and "are for a .blow5 file" in r.stderr, bad
    # accepted names reach the next check, the model that is not there; "none" is accepted for an ASCII file
    for good, out in ((["--compress", "zlib", "--sig_compress", "svb-zd", "-t", "64"], "a.blow5"), (["--compress", "none", "--sig_compress", "none"], "a.slow5")):
        r = simulate(good + ["-o", tmp_path / out, model, ref])
        assert r.returncode == 1 and "cannot open the model" in r.stderr, good
    assert not list(tmp_path.iterdir())
    h = simulate(["-h"]).stdout
    assert "--compress" in h and "--sig_compress" in h and "-t INT" in h
