"""Shared by the tests of the move-table expansion (pg_mvops_*): reads that sit on the edges of the kernels' shapes, batches of them laid
out as the ABI takes them, and a small reader of SAM / BAM records' mv, ns and ts tags. Nothing here calls the product."""
import gzip
import struct

import numpy as np

import kfreq_reads_cases as K
import mvops_ref as R


class Rd:
    """One read: table elements (int8), stride, ns, ts, 4-bit base codes, SAM flag."""

    def __init__(self, mv, stride, ns, ts, codes, flag=0, name=""):
        self.mv = np.asarray(mv, np.int8)
        self.stride, self.ns, self.ts, self.flag, self.name = int(stride), int(ns), int(ts), int(flag), name
        self.codes = np.asarray(codes, np.uint8)

    def ref(self, flags=0):
        return R.expand([int(x) for x in self.mv], self.stride, self.ns, self.ts, self.codes, self.flag, flags)


def _codes(rng, n, n_rate=0.0):
    c = np.array([K.A, K.C_, K.G, K.T], np.uint8)[rng.integers(0, 4, n)]
    if n_rate and n:
        c[rng.random(n) < n_rate] = K.N
    return c


def table(rng, n, first=0, density=0.4):
    """n elements, the first move at element `first` (0-based), moves behind it with the given density."""
    mv = (rng.random(n) < density).astype(np.int8)
    mv[:first] = 0
    if first < n:
        mv[first] = 1
    return mv


def good(rng, mv, stride=5, ts=17, extra=3, L=None, flag=0, n_rate=0.0, name=""):
    """A read reform accepts: as many bases as moves (unless L is given) and a signal that ends `extra` samples behind the table."""
    mv = np.asarray(mv, np.int8)
    m = int((mv == 1).sum())
    ns = (len(mv) - 1) * stride + ts + extra
    return Rd(mv, stride, ns, ts, _codes(rng, m if L is None else L, n_rate), flag, name)


def edge_reads(P, seed=1):
    """[(label, Rd)]: the shapes at which the rule or the kernels take another path; P is the library's piece size."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (1, 2, 63, 64, 65, 127, 128, 129, P - 1, P, P + 1, 2 * P + 1):
        out.append((f"n{n}", good(rng, table(rng, n), stride=(1, 5, 6, 10)[n % 4])))
    out.append(("n1_no_bases", good(rng, [1], L=0)))
    out.append(("n1_one_base", good(rng, [1], L=1)))                           # the only move is the final element: refused
    out.append(("first_at_0", good(rng, table(rng, 200, first=0))))
    out.append(("first_at_1", good(rng, table(rng, 200, first=1))))
    out.append(("first_behind_70_zeros", good(rng, table(rng, 300, first=70), stride=10)))
    mv = table(rng, 150); mv[-1] = 1
    out.append(("move_on_final_element", good(rng, mv)))
    mv = table(rng, P + 7); mv[-1] = 1
    out.append(("move_on_final_element_of_second_piece", good(rng, mv, stride=6)))
    mv = np.zeros(3 * P + 10, np.int8); mv[[3, P - 3, 2 * P + 5, 2 * P + 6, 3 * P + 9]] = 1
    out.append(("zeros_span_a_piece", good(rng, mv, stride=10)))
    mv = np.zeros(2 * P + 100, np.int8); mv[0] = 1; mv[2 * P + 50] = 1
    out.append(("zeros_span_a_piece_from_element_0", good(rng, mv)))
    mv = np.zeros(100, np.int8); mv[0] = 1
    out.append(("only_first_element", good(rng, mv)))
    mv = np.zeros(P + 100, np.int8); mv[0] = 1
    out.append(("only_first_element_long", good(rng, mv, stride=1)))
    mv = table(rng, 400)
    out.append(("more_moves_than_bases", good(rng, mv, L=int((mv == 1).sum()) - 5)))
    mv = table(rng, P + 300)
    out.append(("more_moves_than_bases_cut_in_piece_0", good(rng, mv, L=70)))
    out.append(("one_base_fewer_than_moves", good(rng, mv, L=int((mv == 1).sum()) - 1)))
    mv = table(rng, 400)
    out.append(("fewer_moves_than_bases", good(rng, mv, L=int((mv == 1).sum()) + 1)))
    out.append(("ns_too_small", good(rng, table(rng, 90), extra=-1)))
    out.append(("ns_just_enough", good(rng, table(rng, 90), extra=0)))
    out.append(("ns_too_small_but_no_tail", good(rng, mv, L=10, extra=-50)))   # more moves than bases: the tail is never computed
    out.append(("all_zero", good(rng, np.zeros(130, np.int8), L=4)))
    out.append(("all_zero_long", good(rng, np.zeros(P + 1, np.int8), L=4)))
    out.append(("no_bases", good(rng, table(rng, 50), L=0)))
    mv = table(rng, 64, density=0.5)
    if int((mv == 1).sum()) % 2 == 0:
        mv[np.flatnonzero(mv == 0)[0]] = 1
    out.append(("odd_l_seq", good(rng, mv)))
    for s in (1, 5, 6, 10):
        out.append((f"stride{s}", good(rng, table(rng, 333), stride=s, ts=1000 + s)))
    out.append(("stride0", good(rng, table(rng, 40), stride=0)))
    out.append(("stride_negative", good(rng, table(rng, 40), stride=-5)))
    mv = table(rng, 500); mv[mv == 0] = np.array([0, 2, -1, -127, 3], np.int8)[rng.integers(0, 5, int((mv == 0).sum()))]
    out.append(("elements_other_than_0_and_1", good(rng, mv)))
    out.append(("wrap_around", Rd(table(rng, 100), 0x7fffffff, 5, 3, _codes(rng, 3))))   # uint32 gaps wrap; ns - (...) stays reform's
    mv = table(rng, 260)
    out.append(("reverse", good(rng, mv, flag=0x10, n_rate=0.1)))
    out.append(("reverse_odd", good(rng, mv, flag=0x10, L=int((mv == 1).sum()) - 1 - int((mv == 1).sum()) % 2, n_rate=0.1)))
    out.append(("with_n", good(rng, table(rng, 260), n_rate=0.3)))
    every = good(rng, table(rng, 40, density=1.0), L=16); every.codes = np.arange(16, dtype=np.uint8)
    out.append(("every_code", every))
    every_r = good(rng, table(rng, 40, density=1.0), L=16, flag=0x10); every_r.codes = np.arange(16, dtype=np.uint8)
    out.append(("every_code_reverse", every_r))
    return out


def alignment_reads(seed=2):
    """32 reads back to back whose tables start at every residue mod 16 (lengths of 16 a + 1) twice over."""
    rng = np.random.default_rng(seed)
    return [good(rng, table(rng, 16 * (2 + i % 5) + 1), stride=(5, 10)[i & 1], flag=0x10 if i % 7 == 3 else 0) for i in range(32)]


def layout(reads, lead=0, seq_gaps=(0,), seq_lead=0):
    """The ABI's arrays: mv bytes back to back behind `lead` bytes of 1 (which belong to no read), mv_off, stride, ns, ts, l_seq, flag,
    seq_bytes, byte_off."""
    mv = np.concatenate([np.full(lead, 1, np.int8)] + [r.mv for r in reads]) if reads else np.zeros(lead, np.int8)
    off = np.cumsum([lead] + [len(r.mv) for r in reads]).astype(np.uint64)
    seq, byte_off, l_seq, _ = K.layout([(r.codes, False) for r in reads], seq_gaps, lead=seq_lead)
    return dict(mv=mv, mv_off=off, stride=np.array([r.stride for r in reads], np.int32), ns=np.array([r.ns & 0xffffffffffffffff for r in reads], np.uint64),
                ts=np.array([r.ts & 0xffffffffffffffff for r in reads], np.uint64), l_seq=l_seq.astype(np.uint32), flag=np.array([r.flag for r in reads], np.uint32),
                seq_bytes=seq, byte_off=byte_off.astype(np.uint64))


def expected(reads, flags=0):
    """What the expansion must return for the batch: dict of numpy arrays in the layout of the result."""
    refs = [r.ref(flags) for r in reads]
    ops = [x for f in refs for x in f.ops]
    return dict(status=np.array([f.status for f in refs], np.uint32),
                op_n=np.array(ops, np.uint32), op_off=np.cumsum([0] + [len(f.ops) for f in refs]).astype(np.uint64),
                query_start=np.array([f.query_start for f in refs], np.int32), target_start=np.array([f.target_start for f in refs], np.int32),
                target_end=np.array([f.target_end for f in refs], np.int32),
                seq=np.frombuffer(b"".join(f.seq for f in refs), np.uint8), seq_off=np.cumsum([0] + [len(f.seq) for f in refs]).astype(np.uint64))


# ---- the mv / ns / ts tags of SAM and BAM records, parsed here -------------------------------------------------------------------

def sam_records(path):
    """[(qname, flag, SEQ bytes, stride, [elements], ns, ts)] of a SAM file's records that carry all three tags."""
    out = []
    for line in open(path, "rb").read().split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        c = line.rstrip(b"\r").split(b"\t")
        tags = {t[:2]: t for t in c[11:]}
        if not all(k in tags for k in (b"mv", b"ns", b"ts")):
            continue
        mv = [int(x) for x in tags[b"mv"].split(b",")[1:]]
        out.append((c[0].decode(), int(c[1]), c[9], mv[0], mv[1:], int(tags[b"ns"][5:]), int(tags[b"ts"][5:])))
    return out


_AUX = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
_FMT = {b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I", b"f": "f"}


def bam_records(path):
    """The same of a BAM file (gzip + struct; SEQ as the letters of its codes)."""
    d = gzip.decompress(open(path, "rb").read())
    assert d[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, p)
        p += 8 + l_name
    out = []
    while p < len(d):
        block_size, = struct.unpack_from("<i", d, p)
        end = p + 4 + block_size
        l_read_name, = struct.unpack_from("<B", d, p + 12)
        n_cigar, flag, l_seq = struct.unpack_from("<HHi", d, p + 16)
        q = p + 36
        qname = d[q:q + l_read_name - 1].decode()
        q += l_read_name + 4 * n_cigar
        b = np.frombuffer(d, np.uint8, (l_seq + 1) // 2, q)
        codes = np.stack([b >> 4, b & 15], 1).reshape(-1)[:l_seq]
        q += (l_seq + 1) // 2 + l_seq
        tags = {}
        while q < end:
            tag, ty = d[q:q + 2], d[q + 2:q + 3]
            q += 3
            if ty == b"Z":
                e = d.index(b"\0", q); tags[tag] = d[q:e]; q = e + 1
            elif ty == b"B":
                sub = d[q:q + 1]; cnt, = struct.unpack_from("<i", d, q + 1)
                tags[tag] = (sub, list(struct.unpack_from("<%d%s" % (cnt, _FMT[sub]), d, q + 5))); q += 5 + cnt * _AUX[sub]
            else:
                tags[tag] = struct.unpack_from("<" + _FMT.get(ty, "B"), d, q)[0]; q += _AUX[ty]
        if all(k in tags for k in (b"mv", b"ns", b"ts")):
            mv = tags[b"mv"][1]
            out.append((qname, flag, bytes(K.LETTERS[c] for c in codes), mv[0], mv[1:], int(tags[b"ns"]), int(tags[b"ts"])))
        p = end
    return out
