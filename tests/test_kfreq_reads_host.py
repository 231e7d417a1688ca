"""`poregen kmer_freq` on SAM/BAM input, the parts that need no GPU: the two 16-entry code tables the kernel and the SAM front-end
share (pg_kfreq_codes.h, through _pg_hosttest.so) against the tables written out below, the refusals that come before the device is
opened, and the test helpers (tests/kfreq_reads_cases.py) against hand-derived answers."""
import ctypes as C
import os
import subprocess

import kfreq_reads_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
READ0 = os.path.join(ROOT, "tests", "golden", "single_read", "read_0.fastq")

# SAM specification 4.2.3 / htslib's seq_nt16_str, and the code of the complementary base set
LETTER_OF_CODE = ["=", "A", "C", "M", "G", "R", "S", "V", "T", "W", "Y", "H", "K", "D", "B", "N"]
COMPLEMENT_OF = {"=": "=", "A": "T", "C": "G", "M": "K", "G": "C", "R": "Y", "S": "S", "V": "B",
                 "T": "A", "W": "W", "Y": "R", "H": "D", "K": "M", "D": "H", "B": "V", "N": "N"}


def hosttest():
    return C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))


def kf(*args):
    return subprocess.run([BIN, "kmer_freq"] + [str(a) for a in args], capture_output=True)


def test_letter_and_complement_tables():
    h = hosttest()
    for code, letter in enumerate(LETTER_OF_CODE):
        assert chr(h.pgt_kf_letter(code)) == letter
        assert LETTER_OF_CODE[h.pgt_kf_complement(code)] == COMPLEMENT_OF[letter]
        assert h.pgt_kf_complement(h.pgt_kf_complement(code)) == code
        assert K.LETTERS[code] == ord(letter) and LETTER_OF_CODE[K.COMPLEMENT[code]] == COMPLEMENT_OF[letter]   # the helpers agree


def test_sam_packing_table():
    h = hosttest()
    want = {ord(letter): code for code, letter in enumerate(LETTER_OF_CODE)}
    want.update({ord(letter.lower()): code for code, letter in enumerate(LETTER_OF_CODE) if letter != "="})
    for byte in range(256):
        assert h.pgt_kf_code_of_byte(byte) == want.get(byte, 15), byte     # '#', '*', '.', 'U', digits, NUL: all N
        assert K.code_of_byte(byte) == want.get(byte, 15)


def test_helpers_by_hand():
    codes = K.codes_of(b"AcgN#=m")
    assert list(codes) == [1, 2, 4, 15, 15, 0, 3]
    assert K.pack(codes) == bytes([0x12, 0x4f, 0xf0, 0x3f])                # odd length: the padding nibble is set
    assert K.printed(codes) == b"ACGNN=M"
    assert K.printed(codes, reverse=True) == b"K=NNCGT"
    assert K.printed(codes, reverse=True, n_to_t=True) == b"K=TTCGT"
    assert K.count_printed([b"ACGNN", b"AC", b""], 2) == {b"AC": 2, b"CG": 1, b"GN": 1, b"NN": 1}
    dense, keys, counts = K.split_counter(K.count_printed([b"ACGNN", b"AC"], 2), 2)
    assert dense[1] == 2 and dense[6] == 1 and dense.sum() == 3 and keys == [b"GN", b"NN"] and counts == [1, 1]


def test_n_to_t_is_refused_for_fastq(tmp_path):
    out = tmp_path / "o.txt"
    out.write_text("old")
    r = kf("--n_to_t", "-o", out, 6, READ0)
    assert r.returncode == 1 and r.stdout == b"" and b"--n_to_t applies to .bam and .sam input only" in r.stderr
    assert out.read_text() == "old"                                        # refused before anything is opened
    assert b"--n_to_t" in kf("-h").stdout


def test_bam_with_a_bad_magic_is_refused(tmp_path):
    recs = [(b"a", 0, K.codes_of(b"ACGT")), (b"b", 0, K.codes_of(b"ACGTACGT"))]
    cases = {"magic.bam": K.bam_file(recs, magic=b"BAM\2"), "text.bam": open(READ0, "rb").read(), "empty.bam": b"",
             "gzip.bam": b"\x1f\x8b\x08\0" + b"\0" * 20}
    for name, data in cases.items():
        f = tmp_path / name
        f.write_bytes(data)
        r = kf(6, f)
        assert r.returncode == 1 and r.stdout == b"", name
        assert r.stderr.count(b"ERROR") == 1 and (b"not a BAM file" in r.stderr or b"corrupt BGZF block" in r.stderr), (name, r.stderr)
        assert b"no CPU fallback" not in r.stderr                           # refused before the device is opened
