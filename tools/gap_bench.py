#!/usr/bin/env python3
"""gap_bench.py -- the all-matches and the gapped submits of fit and realign (pg_fit_submit, pg_realign_submit) on one MI355X.

  One process loads one build of libpgmove.so (--lib: another build, e.g. the parent commit's, for an A/B on the same box: run the two
  alternately and take the spread one build shows against itself as the margin). The batch is tools/fit_bench.py's configs[1] shape
  (--reads x --read-samples, signal that follows the model, k = 5) in HBM. Per repetition behind one warm-up:
    fit_pass1_ms / fit_pass2_ms   HIP-event time of k_fit_sums / k_fit_resid (pg_fit_pass_ms)
    fit_submit_ms                 wall time of ModelFit.submit
    realign_align_ms              HIP-event time of k_rl_align (band 10)
    realign_submit_ms             wall time of Realigner.submit
  With --gapped (a build that has PG_BATCH_GAPPED) the same numbers for the same batch with 5 % edits: 2.5 % of the ops turned into an
  I (their base leaves the slice) and a D of 1 to 3 columns put behind another 2.5 % (random bases enter the slice), flagged gapped.
Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def with_edits(hb, rate, seed=2):
    """The host batch with `rate` of its ops edited, as a gapped batch over the reference slices the edits imply."""
    from poregen_amd.engine import Batch
    rng = np.random.default_rng(seed)
    n_ops = hb.op_n.size
    x = rng.random(n_ops)
    is_i = x < rate / 2
    d_cols = np.where((x >= rate / 2) & (x < rate), rng.integers(1, 4, n_ops), 0).astype(np.int64)
    old_off = hb.op_off.astype(np.int64)
    is_i[old_off[1:] - 1] = False; d_cols[old_off[1:] - 1] = 0               # a read ends on a match
    at = np.flatnonzero(d_cols)
    op_n = np.insert(hb.op_n, at + 1, d_cols[at].astype(np.uint32))
    op_t = np.insert(np.where(is_i, 1, 0).astype(np.uint8), at + 1, np.uint8(2))
    added = np.concatenate([[0], np.cumsum(d_cols > 0)])
    op_off = (old_off + added[old_off]).astype(np.uint64)
    cols = (1 - is_i.astype(np.int64)) + d_cols                              # the columns every original op leaves in the slice: its own base, the D behind it
    start = np.concatenate([[0], np.cumsum(cols)])
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(start[-1]))]
    keep = ~is_i
    seq[start[:-1][keep]] = hb.seq[keep]
    return Batch(n_reads=hb.n_reads, sig=hb.sig, sig_off=hb.sig_off, digitisation=hb.digitisation, offset=hb.offset, range=hb.range, query_start=hb.query_start,
                 target_start=hb.target_start, target_end=hb.target_end, seq=seq, seq_off=start[old_off].astype(np.uint64), op_n=op_n, op_t=op_t, op_off=op_off, gapped=True)


def timed(hb, levels, k, reps):
    import torch
    from poregen_amd.engine import ModelFit, Realigner
    db = hb.to_device("cuda:0")
    fit = ModelFit(levels, k)
    ra = Realigner(levels, k, band=10, min_len=3)
    out = dict(fit_pass1_ms=[], fit_pass2_ms=[], fit_submit_ms=[], realign_align_ms=[], realign_submit_ms=[])
    try:
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fr = fit.submit(db)
            t1 = time.perf_counter()
            p1, p2 = fit.pass_ms()
            fit.finish()
            t2 = time.perf_counter()
            got = ra.submit(db, fr, copy=False)
            t3 = time.perf_counter()
            al = ra.kernel_ms()
            if i:
                out["fit_pass1_ms"].append(p1); out["fit_pass2_ms"].append(p2); out["fit_submit_ms"].append((t1 - t0) * 1e3)
                out["realign_align_ms"].append(al); out["realign_submit_ms"].append((t3 - t2) * 1e3)
        out.update(reads=hb.n_reads, samples=int(hb.sig_off[-1]), ops=int(hb.op_off[-1]), fitted_reads=int((fr.status == 0).sum()), n_moved=int(got.n_moved.sum()))
    finally:
        ra.close(); fit.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-samples", type=int, default=4000)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--gapped", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lib:
        from poregen_amd import _abi
        _abi.LIB_PATH = os.path.abspath(args.lib)
    import fit_bench
    k = 5
    levels = np.random.default_rng(k).integers(60000, 130000, 4 ** k).astype(np.uint32)
    hb = fit_bench.make_batch(np.full(args.reads, args.read_samples, np.int64), levels, k)
    out = {"lib": args.lib or "this tree", "all_matches": timed(hb, levels, k, args.reps)}
    if args.gapped:
        out["gapped_5_percent_edits"] = timed(with_edits(hb, 0.05), levels, k, args.reps)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
