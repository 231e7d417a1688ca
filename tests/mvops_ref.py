"""The per-read rule of the move-table expansion (pg_mvops_*), restated in Python from host/reform_cli.cpp (reform_record with k = 1,
m = 0) and from `samtools fastq`'s documented printing of a record. The reference's own reform goldens pin THIS file
(tests/test_mvops_host.py); the header the kernels compile (csrc/pg_mvops.h) is then checked against it. Nothing here calls the product."""
from dataclasses import dataclass
from typing import List

import kfreq_reads_cases as K

OK, NO_MOVE, NEG_TAIL, BASES_LEFT, STRIDE = 0, 1, 2, 3, 4
RNA, N_TO_T = 1, 2                 # PG_MVOPS_RNA, PG_MVOPS_N_TO_T
M32 = 0xffffffff


def _i64(x):
    x &= 0xffffffffffffffff
    return x - (1 << 64) if x >> 63 else x


def _i32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


@dataclass
class Read:
    status: int
    ops: List[int]
    query_start: int
    target_start: int
    target_end: int
    seq: bytes


def expand(mv, stride, ns, ts, codes, flag=0, flags=0) -> Read:
    """mv: the table's elements behind the stride element (ints, -128..127); codes: the record's 4-bit base codes."""
    L = len(codes)
    seq = K.printed(codes, reverse=bool(flag & 0x10), n_to_t=bool(flags & N_TO_T))
    t0, t1 = (L, 0) if flags & RNA else (0, L)
    refused = lambda st: Read(st, [], 0, t0, t1, seq)
    if stride < 1:
        return refused(STRIDE)
    len_mv = len(mv) + 1                                   # bam_auxB_len: the stride element counts
    pos = [i for i in range(1, len_mv) if mv[i - 1] == 1]  # 1-based positions of the moves
    if len(pos) < 1:
        return refused(NO_MOVE)
    ns, ts = _i64(ns), _i64(ts)
    n_kmers = L
    first = pos[0]
    body = first + 1 <= len_mv - 1
    qs = _i32(ts + (first - 1) * stride)
    ops, prev = [], first
    for p in pos[1:]:
        if n_kmers == 0:
            break
        ops.append(((p - prev) * stride) & M32)
        prev = p
        n_kmers -= 1
    if body and n_kmers > 0:
        last = len_mv - 1
        tail = ns - ((((last - 1) * stride) & M32) + ts)
        if tail < 0:
            return refused(NEG_TAIL)
        n_kmers -= 1
        ops.append(((((last - prev) * stride) & M32) + tail) & M32)
    if n_kmers != 0:
        return refused(BASES_LEFT)
    return Read(OK, ops, qs, t0, t1, seq)


def ss_of(ops) -> str:
    return "".join("%d," % x for x in ops)
