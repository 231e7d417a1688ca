"""Restatement of the F1-score metric (the reference's src/f1_score/f1score.py) on SAM text, one signal point at a time with numpy: the
yardstick `poregen f1_score` and engine.AlignmentScorer are compared with. Rules:
  1. records: kept when flags 0x100 and 0x10 are clear; every kept record of both files carries ss and si as Z tags, or the run fails.
  2. dicts: name -> record, first position, last record; pairs in file 1's order; --read_id skips without counting; names missing in
     file 2 count; stop when the count equals read_limit.
  3. si: split on ',', every field int(), at least 4; first signal si[0], first ref si[2] (DNA and RNA), base_shift on side 2.
  4. ss: non-empty, last byte not a digit; "<n>," n points at ref then ref += dir; "<n>I" n points at -1; "<n>D" ref += dir * n.
  5. overlap of the two signal ranges; region skip when START > r1 + 1 or END < r1 + 1; TN / FP / FN on the value -1, then TP or FP.
  6. metrics in double, zero denominators 0.0.
  7. --region: commas removed, CHR:START-END; records on CHR with pos < END and endpos > START."""
import re

import numpy as np


class F1Error(Exception):
    pass


def py_int(s: str) -> int:
    return int(s)  # Python's own rules: whitespace, sign, single underscores


def parse_sam(path):
    refs, recs = [], []
    for line in open(path, "rb").read().split(b"\n"):
        if not line:
            continue
        if line.startswith(b"@"):
            if line.startswith(b"@SQ\t"):
                for f in line.split(b"\t")[1:]:
                    if f.startswith(b"SN:"):
                        refs.append(f[3:].decode())
            continue
        c = line.split(b"\t")
        tags = {}
        for t in c[11:]:
            k, ty, v = t.split(b":", 2)
            tags.setdefault(k.decode(), (ty.decode(), v))
        cig = c[5].decode()
        rlen = 0
        if cig != "*":
            for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cig):
                rlen += int(n) if op in "MDN=X" else 0
        flag = int(c[1])
        pos = int(c[3]) - 1
        end = pos + (1 if (flag & 4) or rlen == 0 else rlen)
        recs.append(dict(name=c[0].decode(), flag=flag, rname=c[2].decode(), pos=pos, endpos=end, tags=tags))
    return refs, recs


def parse_region(region):
    try:
        chrom, positions = region.replace(",", "").split(":")
        start, end = map(int, positions.split("-"))
        return chrom, start, end
    except ValueError:
        raise F1Error("Region must be in the format 'chr:start-end'.")


def load_dict(path, region=None):
    refs, recs = parse_sam(path)
    if region:
        chrom, start, end = parse_region(region)
        if chrom not in refs:
            raise F1Error("invalid contig")
        if start < 0 or start > end:
            raise F1Error("invalid coordinates")
        recs = [r for r in recs if r["rname"] == chrom and r["pos"] < end and r["endpos"] > start]
    d = {}
    for r in recs:
        if r["flag"] & 0x100 or r["flag"] & 0x10:
            continue
        for t in ("ss", "si"):
            if t not in r["tags"] or r["tags"][t][0] != "Z":
                raise F1Error(f"'{t}' tag not found in record with read ID {r['name']}")
        d[r["name"]] = (r["tags"]["ss"][1], r["tags"]["si"][1].decode())
    return d


def expand_ops(n, k, sig0: int, ref0: int, direction: int):
    """expand() on the ops themselves: counts n and kind bytes k as int64 arrays"""
    match, ins, dele = k == ord(","), k == ord("I"), k == ord("D")
    step = np.where(match, 1, np.where(dele, n, 0))
    ref_at = ref0 + direction * (np.cumsum(step) - step)  # ref before each op
    pts = np.where(match | ins, n, 0)
    refs = np.repeat(np.where(ins, -1, ref_at), pts)
    return sig0, refs


def expand(ss: bytes, sig0: int, ref0: int, direction: int):
    """signal positions (contiguous from sig0) and their refs"""
    if not ss or ss[-1:].isdigit():
        raise F1Error("Invalid ss string")
    ops = re.findall(rb"(\d+)(\D)", ss)
    n = np.array([int(a) for a, _ in ops], np.int64)
    k = np.array([b[0] for _, b in ops], np.int64)
    return expand_ops(n, k, sig0, ref0, direction)


def compare(a, b, threshold=0, region=None):
    s1, r1 = a
    s2, r2 = b
    if r1.size == 0 or r2.size == 0:
        raise F1Error("list index out of range")
    lo, hi = max(s1, s2), min(s1 + r1.size, s2 + r2.size)
    if hi <= lo:
        return np.zeros(4, np.int64)
    x, y = r1[lo - s1:hi - s1], r2[lo - s2:hi - s2]
    if region is not None:
        keep = ~((region[0] > x + 1) | (region[1] < x + 1))
        x, y = x[keep], y[keep]
    tn = int(((x == -1) & (y == -1)).sum())
    fp = int(((x == -1) & (y != -1)).sum())
    fn = int(((x != -1) & (y == -1)).sum())
    close = np.abs(x - y) <= threshold
    return np.array([int(close.sum()), fp + int((~close).sum()), tn, fn], np.int64)


def pair_counts(ss1, si1, ss2, si2, rna=False, threshold=0, base_shift=0, region=None):
    a = tuple(py_int(v) for v in si1.split(","))
    b = tuple(py_int(v) for v in si2.split(","))
    if len(a) < 4 or len(b) < 4:
        raise F1Error("tuple index out of range")
    d = -1 if rna else 1
    return compare(expand(ss1, a[0], a[2], d), expand(ss2, b[0], b[2] + base_shift, d), threshold, region)


def pair_counts_py(ss1, sig1, ref1, ss2, sig2, ref2, rna=False, threshold=0, region=None):
    """pair_counts on Python ints, one point at a time as f1score.py walks them (parse_ss_string :19-57, compare_mappings :89-116):
    for values whose sums or differences leave int64. ss as bytes, the scalars as ints (side 2's ref with base_shift added)."""
    maps = []
    for ss, sig, ref in ((ss1, sig1, ref1), (ss2, sig2, ref2)):
        if not ss or ss[-1:].isdigit():
            raise F1Error("Invalid ss string")
        m, num = {}, ""
        for ch in ss.decode("ascii"):
            if ch.isdigit():
                num += ch
                continue
            if num:
                n = int(num)
                if ch == ",":
                    for _ in range(n):
                        m[sig] = ref
                        sig += 1
                    ref += -1 if rna else 1
                elif ch == "D":
                    ref += -n if rna else n
                elif ch == "I":
                    for _ in range(n):
                        m[sig] = -1
                        sig += 1
            num = ""
        if not m:
            raise F1Error("list index out of range")
        maps.append(m)
    tp = fp = tn = fn = 0
    for sig in sorted(maps[0].keys() & maps[1].keys()):  # both ranges are contiguous: the common keys are the overlap
        r1, r2 = maps[0][sig], maps[1][sig]
        if region is not None and (region[0] > r1 + 1 or region[1] < r1 + 1):
            continue
        if r1 == -1 and r2 == -1:
            tn += 1
        elif r1 == -1:
            fp += 1
        elif r2 == -1:
            fn += 1
        if abs(r1 - r2) <= threshold:
            tp += 1
        else:
            fp += 1
    return [tp, fp, tn, fn]


def metrics(tp, fp, tn, fn):
    p = tp / (tp + fp) if tp + fp > 0 else 0.0
    r = tp / (tp + fn) if tp + fn > 0 else 0.0
    f1 = 2 * (p * r) / (p + r) if p + r > 0 else 0.0
    sp = tn / (tn + fp) if tn + fp > 0 else 0.0
    acc = (tp + tn) / (tp + fp + tn + fn) if tp + fp + tn + fn > 0 else 0.0
    return p, r, f1, sp, acc


def run(bam1, bam2, read_limit=100, base_shift=0, read_id=None, region=None, rna=False, threshold=0, with_pairs=False):
    """stdout of `f1score.py bam1 bam2 ...` as bytes (SAM text inputs), or F1Error"""
    d1 = load_dict(bam1, region)
    d2 = load_dict(bam2, region)
    reg = parse_region(region)[1:] if region else None
    tot = np.zeros(4, np.int64)
    per = []
    count = 0
    for name in d1:
        if read_id and name != read_id:
            continue
        if name in d2:
            try:
                c = pair_counts(d1[name][0], d1[name][1], d2[name][0], d2[name][1], rna, threshold, base_shift, reg)
            except (F1Error, ValueError) as e:
                raise F1Error(f"read {name}: {e}")
            tot += c
            per.append(c)
        count += 1
        if read_limit is not None and count == read_limit:
            break
    tp, fp, tn, fn = (int(v) for v in tot)
    m = metrics(tp, fp, tn, fn)
    out = "TP\tFP\tTN\tFN\t%d\t%d\t%d\t%d\n" % (tp, fp, tn, fn)
    out += "precision\trecall\tF1_score\tspecificity\taccuracy\t" + "\t".join(f"{v:.3f}" for v in m) + "\n"
    return (out.encode(), per) if with_pairs else out.encode()
