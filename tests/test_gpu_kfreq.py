"""`poregen kmer_freq` on the MI355X: the CLI's output byte for byte against tests/kfreq_ref.py, and the counter's Python API on
pieces cut anywhere, on device-resident input, past 2^32 in one bin, and across reuse and errors."""
import os
import subprocess

import numpy as np
import pytest

import kfreq_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
READ0 = os.path.join(ROOT, "tests", "golden", "single_read", "read_0.fastq")


def kf(*args, env=None):
    e = dict(os.environ, **(env or {}))
    return subprocess.run([BIN, "kmer_freq"] + [str(a) for a in args], capture_output=True, env=e)


def synth_fastq(n_reads, seed, alphabet=b"ACGT", mean_len=300, n_rate=0.0, crlf=False):
    rng = np.random.default_rng(seed)
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n_reads):
        L = int(rng.integers(0, 2 * mean_len))
        s = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), L)].copy()
        if n_rate:
            s[rng.random(L) < n_rate] = ord("N")
        q = (rng.integers(33, 74, L)).astype(np.uint8)
        out += [b"@read_%d runid=x" % i, s.tobytes(), b"+", q.tobytes()]
    return nl.join(out) + nl


def check_cli(tmp_path, data, k, sort=0, absent=1, env=None):
    f = tmp_path / "in.fastq"
    f.write_bytes(data)
    r = kf("--sort", sort, "--print_absent_kmers", absent, k, f, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == R.expected(data, k, sort, absent)
    return r


# ---- the CLI ---------------------------------------------------------------------------------------------------------------

def test_reference_command_lines(tmp_path):
    data = open(READ0, "rb").read()
    # test_kmer_freq.sh: 1 (no args) ... 6, plus --sort 2
    assert kf().returncode == 1
    cases = [[], ["--print_absent_kmers", 0], ["--print_absent_kmers", 0, "--sort", 1], ["--print_absent_kmers", 1, "--sort", 1],
             ["--print_absent_kmers", 0, "--sort", 1], ["--print_absent_kmers", 0, "--sort", 2], ["--sort", 2]]
    for i, extra in enumerate(cases):
        out = tmp_path / f"{i}.txt"
        r = kf(6, READ0, "-o", out, *extra)
        assert r.returncode == 0, r.stderr
        opts = dict(zip(extra[::2], extra[1::2]))
        want = R.expected(data, 6, int(opts.get("--sort", 0)), int(opts.get("--print_absent_kmers", 1)))
        assert out.read_bytes() == want and r.stdout == b""
        assert b"kmer_size: 6\nnum_kmers: 4096\n" in r.stderr
    r = kf(6, READ0, "--print_absent_kmers", 0)
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 53 and sum(int(x.split("\t")[1]) for x in lines) == 476


@pytest.mark.parametrize("k", range(1, 13))
def test_every_k_on_synthetic(tmp_path, k):
    data = synth_fastq(300, seed=100 + k, n_rate=0.002)
    check_cli(tmp_path, data, k, sort=k % 3, absent=1 if k <= 7 else 0)


def test_odd_bytes(tmp_path):
    data = synth_fastq(60, seed=3, alphabet=b"ACGTNacgtRYKMSWBDHV", mean_len=80)
    for k in (1, 3, 5, 7):
        check_cli(tmp_path, data, k, sort=k % 3)
    crlf = synth_fastq(80, seed=4, n_rate=0.01, crlf=True)
    for k in (2, 6, 9):
        check_cli(tmp_path, crlf, k, absent=0)


def test_short_and_empty_lines_and_unterminated_ends(tmp_path):
    data = b"@a\nAC\n+\nII\n@b\n\n+\n\n@c\nACGTACGT\n+\nIIIIIIII\n@d\nA\n+\nI\n"
    for k in (1, 2, 3, 5, 9):
        check_cli(tmp_path, data, k, absent=0)
    check_cli(tmp_path, b"@a\nACGTTGCA\n+\nIIIIIIII\n@b\nGGGTTTAAC", 3, absent=0)   # unterminated sequence line
    check_cli(tmp_path, b"@a\nACGTTGCA\n+\nIIIIIIII\n@b\nGGGTTTAAC\n+\nIIIIIIIII", 3, absent=0)   # unterminated quality line
    check_cli(tmp_path, b"\n\n\n\n\nACGT\n", 2, absent=0)   # empty lines count as lines


def test_all_n_overflows_the_odd_list(tmp_path):
    # 3 M windows of one key against a list of 1 M entries (and a second run with the default list)
    data = b"@r\n" + b"N" * 3_000_000 + b"\n+\n" + b"I" * 3_000_000 + b"\n"
    want = R.expected(data, 7, 0, 0)
    f = tmp_path / "n.fastq"
    f.write_bytes(data)
    for env in ({"PGKFREQ_ODD_CAP": "1000000"}, {"PGKFREQ_ODD_CAP": "1000", "POREGEN_KFREQ_PIECE": "65536"}, None):
        r = kf("--print_absent_kmers", 0, 7, f, env=env)
        assert r.returncode == 0 and r.stdout == want == b"NNNNNNN\t2999994\n"


def test_long_read_and_line_longer_than_piece(tmp_path):
    rng = np.random.default_rng(9)
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1_000_000)].tobytes()
    data = b"@long\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"
    check_cli(tmp_path, data, 9, absent=0)
    check_cli(tmp_path, data, 5, env={"POREGEN_KFREQ_PIECE": "4099"})


def test_nul_bytes(tmp_path):
    f = tmp_path / "z.fastq"
    f.write_bytes(b"@r\nACG\0TACGT\n+\nIIIIIIIII\n")
    r = kf(3, f)
    assert r.returncode == 1 and b"NUL" in r.stderr
    check_cli(tmp_path, b"@r\0x\nACGTACGT\n+\nIIIIIIII\n", 3)


# ---- the Python API --------------------------------------------------------------------------------------------------------

def _same(res, data, k):
    c = R.count(data, k)
    want = np.zeros(4 ** k, np.uint64)
    odd = {}
    for key, n in c.items():
        if set(key) <= set(b"ACGT"):
            want[int("".join("ACGT"[b"ACGT".index(x)] for x in key).translate(str.maketrans("ACGT", "0123")), 4)] = n
        else:
            odd[key] = n
    assert np.array_equal(res.counts, want)
    assert res.odd_keys == sorted(odd) and [int(x) for x in res.odd_counts] == [odd[x] for x in sorted(odd)]


def test_every_split_offset():
    from poregen_amd.engine import KmerCounter
    data = b"@a\nACGTNACGTA\n+\nIIIIIIIIII\n@b\nTTGCAACGT"
    for k in (1, 3, 4):
        kc = KmerCounter(k)
        whole = None
        for cut in range(len(data) + 1):
            kc.submit(data[:cut]); kc.submit(data[cut:])
            r = kc.finish()
            _same(r, data, k)
            if whole is None:
                whole = r
        for a in range(0, len(data), 3):   # three pieces
            for b in range(a, len(data), 5):
                kc.submit(data[:a]); kc.submit(data[a:b]); kc.submit(data[b:])
                _same(kc.finish(), data, k)
        kc.close()
    big = synth_fastq(2000, seed=11, n_rate=0.003)
    rng = np.random.default_rng(1)
    kc = KmerCounter(9)
    cuts = np.sort(rng.integers(0, len(big), 40))
    prev = 0
    for c in list(cuts) + [len(big)]:
        kc.submit(np.frombuffer(big[prev:c], np.uint8)); prev = c
    _same(kc.finish(), big, 9)
    kc.close()


def test_device_resident_pieces():
    import torch
    from poregen_amd.engine import KmerCounter, kmer_freq
    data = synth_fastq(3000, seed=12, n_rate=0.002)
    host = kmer_freq(data, 6)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    dev = kmer_freq(t, 6)
    assert np.array_equal(host.counts, dev.counts) and host.odd_keys == dev.odd_keys
    kc = KmerCounter(10)
    for a, b in [(0, 1), (1, 77777), (77777, 77778), (77778, len(data))]:
        kc.submit(t[a:b])   # unaligned device pointers included
    _same(kc.finish(), data, 10)
    kc.close()


def test_homopolymer_past_two_to_the_32():
    import torch
    from poregen_amd.engine import KmerCounter
    n = (1 << 32) + (1 << 20)
    t = torch.full((n,), ord("A"), dtype=torch.uint8, device="cuda")
    t[0] = ord("@"); t[1] = ord("\n"); t[n - 1] = ord("\n")
    torch.cuda.synchronize()
    for k in (5, 9):
        kc = KmerCounter(k)
        kc.submit(t)
        r = kc.finish()
        kc.close()
        assert int(r.counts[0]) == n - 3 - k + 1 and int(r.counts.sum()) == n - 3 - k + 1 and not r.odd_keys
    del t
    torch.cuda.empty_cache()


def test_reuse_and_error_recovery():
    from poregen_amd import _abi
    from poregen_amd.engine import KmerCounter, PgError
    a = synth_fastq(50, seed=20, n_rate=0.01)
    b = synth_fastq(70, seed=21)
    kc = KmerCounter(5)
    kc.submit(a); _same(kc.finish(), a, 5)
    kc.submit(b); _same(kc.finish(), b, 5)             # nothing of `a` leaks
    kc.submit(b"@r\nAC\0GTACGT\n+\nIIIIIIIII\n")
    with pytest.raises(PgError) as ei:
        kc.finish()
    assert ei.value.status == _abi.PG_ERR_INPUT
    kc.submit(a); _same(kc.finish(), a, 5)             # the same counter works afterwards
    kc.close()
    kc = KmerCounter(5)
    kc.submit(b"@r\nACGT"); kc.close()                 # destroyed mid-stream
    kc = KmerCounter(5)
    kc.submit(b); _same(kc.finish(), b, 5)
    kc.close()
