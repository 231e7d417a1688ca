"""The per-read rule of the move-table expansion without a GPU. tests/mvops_ref.py (Python, written from host/reform_cli.cpp) is pinned
by the reference's own reform goldens made with -k 1 -m 0; csrc/pg_mvops.h -- the header the kernels compile -- then runs through
_pg_hosttest.so against mvops_ref.py on the edge cases of tests/mvops_cases.py."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import kfreq_reads_cases as K
import mvops_cases as M
import mvops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "reform")


@pytest.fixture(scope="module")
def h():
    return C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))


def levels(h):
    out = (C.c_uint32 * 3)()
    h.pgt_mvops_levels(out)
    return list(out)


def host_expand(h, rd, flags=0):
    mv = np.ascontiguousarray(rd.mv.view(np.uint8))
    L = len(rd.codes)
    packed = np.frombuffer(K.pack(rd.codes) + b"\xff", np.uint8)
    ops = np.full(L + 1, 0xdeadbeef, np.uint32)
    seq = np.zeros(L + 1, np.uint8)
    n_ops, qs = C.c_uint32(), C.c_int32()
    st = h.pgt_mvops_expand(C.c_void_p(mv.ctypes.data), C.c_uint32(len(mv)), C.c_int32(rd.stride), C.c_uint64(rd.ns), C.c_uint64(rd.ts), C.c_uint32(L),
                            C.c_void_p(packed.ctypes.data), int(bool(rd.flag & 0x10)), int(bool(flags & R.N_TO_T)), C.c_void_p(ops.ctypes.data),
                            C.byref(n_ops), C.byref(qs), C.c_void_p(seq.ctypes.data))
    assert ops[L] == 0xdeadbeef and seq[L] == 0
    return st, [int(x) for x in ops[:n_ops.value]], qs.value, seq[:L].tobytes()


def test_levels():
    lane, step, piece = levels(C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so")))
    assert lane == 16 and step == 64 * lane and piece % step == 0 and piece >= step


def test_mask4(h):
    rng = np.random.default_rng(0)
    words = [0, 0x01010101, 0x00000001, 0x01000000, 0x02010081, 0xff01fe01, 0x00010100, 0x81018101] + [int(x) for x in rng.integers(0, 1 << 32, 2000)]
    words += [int.from_bytes(bytes(rng.integers(0, 3, 4).astype(np.uint8)), "little") for _ in range(2000)]
    for w in words:
        want = sum(1 << i for i in range(4) if (w >> (8 * i)) & 0xff == 1)
        assert h.pgt_mvops_mask4(C.c_uint32(w)) == want, hex(w)


def test_header_against_the_python_rule(h):
    P = levels(h)[2]
    for label, rd in M.edge_reads(P) + [(f"align{i}", r) for i, r in enumerate(M.alignment_reads())]:
        for flags in (0, R.N_TO_T):
            want = rd.ref(flags)
            st, ops, qs, seq = host_expand(h, rd, flags)
            assert st == want.status, label
            assert ops == want.ops, label
            assert seq == want.seq, label
            if st == R.OK:
                assert qs == want.query_start, label


def test_every_status_and_shape_is_among_the_cases(h):
    P = levels(h)[2]
    cases = dict(M.edge_reads(P))
    st = {k: v.ref().status for k, v in cases.items()}
    assert {st["all_zero"], st["ns_too_small"], st["fewer_moves_than_bases"], st["stride0"]} == {R.NO_MOVE, R.NEG_TAIL, R.BASES_LEFT, R.STRIDE}
    assert st["n1_one_base"] == R.BASES_LEFT and st["n1_no_bases"] == R.OK and st["ns_just_enough"] == R.OK and st["ns_too_small_but_no_tail"] == R.OK
    for n in (1, 2, 63, 64, 65, 127, 128, 129, P - 1, P, P + 1, 2 * P + 1):
        assert len(cases[f"n{n}"].mv) == n and (n == 1 or st[f"n{n}"] == R.OK)
    r = cases["more_moves_than_bases"].ref()
    assert r.status == R.OK and len(r.ops) == len(cases["more_moves_than_bases"].codes) < int((cases["more_moves_than_bases"].mv == 1).sum()) - 1
    r = cases["only_first_element"].ref()
    assert r.status == R.OK and r.ops == [99 * 5 + 3] and r.query_start == 17
    assert cases["reverse"].ref().seq == K.printed(cases["reverse"].codes, reverse=True) != K.printed(cases["reverse"].codes)
    assert b"N" in cases["with_n"].ref().seq and b"N" not in cases["with_n"].ref(R.N_TO_T).seq
    assert (cases["n64"].ref(R.RNA).target_start, cases["n64"].ref(R.RNA).target_end) == (len(cases["n64"].codes), 0)
    assert (cases["n64"].ref().target_start, cases["n64"].ref().target_end) == (0, len(cases["n64"].codes))
    starts = np.cumsum([0] + [len(r.mv) for r in M.alignment_reads()])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))


def hand_checked():
    # 12 table elements, moves at positions 1, 3, 6, 7, 12; stride 5, ts 10, ns 100; 5 bases
    mv = [1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1]
    return mv, R.expand(mv, 5, 100, 10, K.codes_of(b"ACGTN"))


def test_python_rule_by_hand():
    mv, r = hand_checked()
    assert r.status == R.OK and r.query_start == 10 and r.ops == [10, 15, 5, 25, 0 * 5 + (100 - (11 * 5 + 10))] and r.seq == b"ACGTN"
    assert R.expand(mv, 5, 100, 10, K.codes_of(b"ACG")).ops == [10, 15, 5]
    assert R.expand(mv, 5, 100, 10, K.codes_of(b"ACGTNA")).status == R.BASES_LEFT
    assert R.expand(mv, 5, 64, 10, K.codes_of(b"ACGTN")).status == R.NEG_TAIL
    assert R.expand(mv, 5, 65, 10, K.codes_of(b"ACGTN")).ops[-1] == 0
    assert R.expand(mv[:11], 5, 100, 10, K.codes_of(b"ACGT")).ops == [10, 15, 5, 4 * 5 + (100 - (10 * 5 + 10))]
    assert R.expand(mv, 5, 100, 10, K.codes_of(b"ACGTN"), flag=0x10, flags=R.N_TO_T | R.RNA).seq == b"TACGT"


def _check_paf(paf_bytes, records):
    lines = paf_bytes.decode().splitlines()
    assert len(lines) == len(records) > 0
    for line, (qname, flag, seq, stride, mv, ns, ts) in zip(lines, records):
        c = line.split("\t")
        r = R.expand(mv, stride, ns, ts, K.codes_of(seq), flag)
        assert r.status == R.OK and c[0] == qname
        assert c[12] == "ss:Z:" + R.ss_of(r.ops)
        assert int(c[2]) == r.query_start and int(c[1]) == ns and int(c[6]) == len(r.ops)


def test_python_rule_reproduces_the_reform_goldens_of_k1_m0():
    _check_paf(open(f"{G}/r1k1m0.paf", "rb").read(), M.bam_records(f"{G}/guppy_one_read.bam"))
    _check_paf(open(f"{G}/dr2k1m0.paf", "rb").read(), M.sam_records(f"{G}/slow5-dorado.sam"))
    # the RNA golden has no input file: its table is rebuilt from the TSV's starts (tests/test_reform_rna.py)
    rows = [l.split("\t") for l in open(f"{G}/rna/rna_2.1.tsv").read().splitlines()]
    mv = [0] * 3615
    for row in rows:
        mv[(int(row[2]) - 9176) // 10] = 1
    paf = open(f"{G}/rna/rna_2.1.paf", "rb").read()
    _check_paf(paf, [(rows[0][0], 4, b"A" * 797, 10, mv, 45325, 9176)])
    r = R.expand(mv, 10, 45325, 9176, K.codes_of(b"A" * 797), 4, R.RNA)
    c = paf.decode().split("\t")
    assert (int(c[7]), int(c[8])) == (r.target_start, r.target_end) == (797, 0) and len(r.ops) == 797 and r.ops[-1] == 9 + 20


def test_gmove_fixture_paf_is_reproduced_too():
    S = os.path.join(ROOT, "tests", "golden", "single_read")
    ref = open(f"{S}/guppy_move.paf").read().rstrip("\n").split("\t")
    for recs in (M.bam_records(f"{S}/guppy_move.bam"), M.sam_records(f"{S}/guppy_move.sam")):
        (qname, flag, seq, stride, mv, ns, ts), = recs
        r = R.expand(mv, stride, ns, ts, K.codes_of(seq), flag)
        assert "ss:Z:" + R.ss_of(r.ops) == [c for c in ref if c.startswith("ss:Z:")][0] and int(ref[2]) == r.query_start
