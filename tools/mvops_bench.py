#!/usr/bin/env python3
"""mvops_bench.py -- the move-table expansion (pg_mvops_expand) and `poregen gmove --reform` on one MI355X.

  device   the batch already in HBM (CUDA tensors, PG_LOC_DEVICE): wall time of MoveExpander.expand -- its five kernels plus the
           read-back of the statuses -- as the best of --reps runs after one warm-up, at the configs[1] shape (50 000 reads x 800 table
           elements) and at a ragged shape (lognormal table lengths from 400 to 200 000 elements, the same total). Bytes per second over
           the bytes the kernels must move at least once (tables read twice, packed bases read, ops + op_t + seq written) beside the
           8 TB/s HBM peak DESIGN.md uses.
  cli      wall time, median of --runs, of `gmove --reform reads.bam` against the two-step route on the same files:
           `reform -c -k 1 --stride 0` plus `gmove --fastq reads.fastq reads.paf`, both commands' times added.
Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def tables(lengths, seed=1, density=0.45):
    """Back-to-back tables of the given lengths, each opened by a move, with as many bases as moves and a signal that ends with the table."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    mv = (rng.random(int(off[-1])) < density).astype(np.int8)
    mv[off[:-1].astype(np.int64)] = 1
    moves = np.add.reduceat(mv.astype(np.int64), off[:-1].astype(np.int64))
    l_seq = moves.astype(np.uint32)
    nb = (l_seq.astype(np.int64) + 1) // 2
    boff = np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64)
    codes = np.array([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88], np.uint8)
    seqb = codes[rng.integers(0, 16, int(boff[-1]))]
    n = len(lengths)
    stride = np.full(n, 10, np.int32)
    ts = np.full(n, 100, np.uint64)
    ns = (np.asarray(lengths, np.uint64) - 1) * 10 + 100 + 7
    return dict(mv=mv, mv_off=off, stride=stride, ns=ns, ts=ts, l_seq=l_seq, flag=np.zeros(n, np.uint32), seq_bytes=seqb, byte_off=boff[:-1].copy())


def bench_device(name, lengths, reps):
    import torch
    from poregen_amd.engine import MoveExpander
    a = tables(lengths)
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    ex = MoveExpander()
    best = None
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ex.expand(t["mv"], t["mv_off"], t["stride"], t["ns"], t["ts"], t["l_seq"], t["flag"], t["seq_bytes"], t["byte_off"], rna=True)
        dt = time.perf_counter() - t0
        if i and (best is None or dt < best):
            best = dt
    assert r.n_refused == 0 and r.n_ops == int(a["l_seq"].sum())
    moved = 2 * a["mv"].size + a["seq_bytes"].size + r.n_ops * (4 + 1 + 1)
    ex.close()
    return dict(shape=name, reads=len(lengths), table_bytes=int(a["mv"].size), ops=int(r.n_ops), seconds=best, bytes_moved=int(moved),
                bytes_per_s=moved / best, share_of_hbm_peak=moved / best / HBM_PEAK)


def bench_cli(n_reads, runs, tmp):
    from poregen_amd import synth
    b = synth.make_batch_fast(n_reads, kind="rna004", seed=11)
    b.target_start = np.zeros_like(b.target_start)
    pre = os.path.join(tmp, "mv")
    synth.write_bam(b, pre + ".bam", block_bytes=60000)
    synth.write_blow5(b, pre + ".blow5")
    with open(pre + ".fastq", "w") as f:
        for r in range(b.n_reads):
            s = synth.seq_string(b, r)
            f.write(f"@r{r}\n{s}\n+\n{'I' * len(s)}\n")
    exe = os.path.join(ROOT, "bin", "poregen")
    opts = ["--rna", "-k", "5", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "1000000", "--index_end", "1023"]   # a slice: every read is read

    def timed(cmd):
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return time.perf_counter() - t0

    one, two, parts = [], [], []
    for i in range(runs + 1):
        for d in ("o1", "o2"):
            shutil.rmtree(os.path.join(tmp, d), ignore_errors=True)
        a = timed([exe, "gmove", "--reform", pre + ".blow5", pre + ".bam"] + opts + [os.path.join(tmp, "o1")])
        r = timed([exe, "reform", "-c", "-k", "1", "--stride", "0", "--rna", "-o", pre + ".paf", pre + ".bam"])
        g = timed([exe, "gmove", "--fastq", pre + ".fastq", pre + ".blow5", pre + ".paf"] + opts + [os.path.join(tmp, "o2")])
        if i:
            one.append(a); two.append(r + g); parts.append((r, g))
    same = subprocess.run(["diff", "-rq", os.path.join(tmp, "o1"), os.path.join(tmp, "o2")], capture_output=True).returncode == 0
    return dict(reads=n_reads, samples=int(b.sig_off[-1]), runs=runs, one_step_median_s=statistics.median(one), two_step_median_s=statistics.median(two),
                reform_median_s=statistics.median(p[0] for p in parts), gmove_paf_median_s=statistics.median(p[1] for p in parts),
                one_step_s=one, two_step_s=two, outputs_equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cli-reads", type=int, default=20000)
    ap.add_argument("--cases", default="device,cli")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {}
    if "device" in args.cases:
        rng = np.random.default_rng(3)
        ragged = np.clip(rng.lognormal(7.6, 1.0, 200000), 400, 200000).astype(np.int64)
        ragged = ragged[:int(np.searchsorted(np.cumsum(ragged), 50000 * 800)) + 1]
        out["device"] = [bench_device("configs[1]: 50000 x 800", np.full(50000, 800, np.int64), args.reps), bench_device("ragged 400..200000", ragged, args.reps)]
    if "cli" in args.cases:
        tmp = tempfile.mkdtemp(prefix="mvops_bench", dir=args.tmp)
        try:
            out["cli"] = bench_cli(args.cli_reads, args.runs, tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
