#!/usr/bin/env python3
"""sigdec_bench.py -- the svb-zd decoder (pg_sigdec_*, csrc/pg_svb.hip) alone on one MI355X.

The configs[1]-shaped batch (50 000 reads x 4 000 samples) and the ragged workload (synth.ragged_lengths, 200 M samples, reads of up to
10^6 samples) are encoded on the host as slow5lib encodes them, the blocks are put into HBM, and SignalDecoder.decode() runs on them
(PG_LOC_DEVICE): best of --reps calls after a warm-up, the synchronise inside the time. A call is offsets and counts to the device, the
kernels, the flags back -- not a kernel figure. For that, run this tool under `rocprofv3 --kernel-trace --stats` and pass the database
as --trace, with the JSON of that run as --table-for, to a second run: per workload the median time of each k_svb_* kernel, and (compressed bytes in + 2 * samples out) over their
sum as a share of the 8 TB/s HBM peak. --max-samples cuts both workloads (a quick look). Prints one JSON object, writes it to --out."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12


def blocks_of(b, synth):
    parts, off = [], [0]
    for r in range(b.n_reads):
        blk = synth._svb_zd(b.sig[int(b.sig_off[r]):int(b.sig_off[r + 1])])
        parts.append(blk); off.append(off[-1] + len(blk))
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint64)


def kernel_table(db, res):
    """the k_svb_* launches of the database, dealt to the workloads in order (each ran warm-up + reps calls)"""
    import sqlite3
    import statistics
    if db.endswith(".csv"):      # rocprofv3 --output-format csv: <name>_kernel_trace.csv
        import csv
        rows = sorted(((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(open(db))))
        rows = [(n, d) for _, n, d in rows]
    else:
        rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    def short(n):
        m = re.search(r"k_svb_[a-z]+(<[a-z0-9_ ]+>)?", n)
        return m.group(0).replace("<true>", "<1>").replace("<false>", "<0>")
    rows = [(short(n), d / 1000) for n, d in rows if "k_svb_" in n]
    out, i = {}, 0
    for name, w in res["device"].items():
        per_call = w["launches_per_call"]
        n = per_call * w["calls"]
        mine, i = rows[i:i + n], i + n
        byk = {}
        for k, d in mine:
            byk.setdefault(k, []).append(d)
        med = {k: round(statistics.median(v), 1) for k, v in byk.items()}
        calls = {k: len(v) for k, v in byk.items()}
        total = sum(statistics.median(v) * (len(v) // w["calls"]) for v in byk.values())
        out[name] = {"kernel_us_median": med, "launches": calls, "sum_us": round(total, 1), "bytes_in_plus_out": w["bytes_in"] + w["bytes_out"],
                     "GBps": round((w["bytes_in"] + w["bytes_out"]) / total / 1e3, 1),
                     "of_hbm_peak": round((w["bytes_in"] + w["bytes_out"]) / (total * 1e-6) / PEAK, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-samples", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigdec_bench.json"))
    ap.add_argument("--trace", help="rocprofv3 database (or kernel-trace csv) of an earlier run of this tool with the same options")
    ap.add_argument("--table-for", help="with --trace: the JSON that run wrote; nothing is measured, the kernel table is added to it (no GPU needed)")
    a = ap.parse_args()
    if a.table_for:
        res = json.loads(open(a.table_for).read())
        res["kernels"] = kernel_table(a.trace, res)
        line = json.dumps(res)
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    import torch
    from poregen_amd import synth
    from poregen_amd.engine import SignalDecoder
    if not torch.cuda.is_available():
        raise SystemExit("sigdec_bench: no GPU (this tool measures the device path; there is no CPU fallback)")
    dec = SignalDecoder()
    res = {"device_name": torch.cuda.get_device_name(0), "peak_hbm_GBps": PEAK / 1e9, "device": {}}
    n1 = 50000 if not a.max_samples else max(1, a.max_samples // 4000)
    lens = synth.ragged_lengths(a.max_samples) if a.max_samples else synth.ragged_lengths()
    for name, make in (("configs1", lambda: synth.make_batch_fast(n1, 4000, seed=20251003)), ("ragged", lambda: synth.make_ragged_fast(lens))):
        b = make()
        blocks, boff = blocks_of(b, synth)
        want = torch.from_numpy(b.sig).cuda()
        d_blocks = torch.from_numpy(blocks).cuda()
        out = torch.empty(b.sig.size, dtype=torch.int16, device="cuda")
        soff = b.sig_off.astype(np.uint64)
        _, _, bad = dec.decode(d_blocks, boff, sig_off=soff, out=out)
        torch.cuda.synchronize()
        assert not bad.any() and torch.equal(out, want)
        best = 1e30
        for _ in range(a.reps):
            torch.cuda.synchronize(); t = time.perf_counter()
            dec.decode(d_blocks, boff, sig_off=soff, out=out)
            torch.cuda.synchronize(); best = min(best, time.perf_counter() - t)
        n_long = int((np.diff(b.sig_off.astype(np.int64)) > 4096).sum())
        res["device"][name] = {"reads": b.n_reads, "samples": int(b.sig.size), "bytes_in": int(blocks.size), "bytes_out": int(b.sig.nbytes),
                               "bytes_per_sample_in": round(blocks.size / b.sig.size, 3), "reads_over_one_piece": n_long,
                               "launches_per_call": 2 + (4 if n_long else 0),      # k_svb_heads, k_svb_decode<1>; a long read: + lens, scan, decode<0>, scan
                               "calls": a.reps + 1, "call_s": round(best, 6),
                               "call_GBps": round((blocks.size + b.sig.nbytes) / best / 1e9, 1)}
        del want, d_blocks, out, b
        torch.cuda.empty_cache()
    if a.trace:
        res["kernels"] = kernel_table(a.trace, res)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
