#!/usr/bin/env python3
"""evalign_bench.py -- the three stages of `poregen eventalign` (pg_evalign_submit) on one MI355X.

  The batch is tools/fit_bench.py's configs[1] shape (50 000 reads of 4 000 samples whose signal follows the model, so that every read is
  fitted and has rows), already in HBM (CUDA tensors, PG_LOC_DEVICE). It is fitted once (ModelFit); then --reps submits after one warm-up:
    count_ms / rows_ms / text_ms   HIP-event time of k_ea_count, of k_ea_rows, and of the text (k_ea_lens, the scan of the lengths, the
                                   host's read of the total that sizes the buffer, k_ea_write), the best of the submits (pg_evalign_kernel_ms)
    rows_per_s                     rows over rows_ms
    text_bytes_per_s               text bytes over text_ms
    rows_read_bytes_per_s          what the rows stage must read at least once (2 bytes per sample, 4 per op, 1 per base) over rows_ms, beside
                                   stream_read_tbps, the best plain streaming read of tools/probe/stream_probe.hip in the same run
    submit_ms                      wall time of the whole call with the rows and the text copied to the host
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
import fit_bench  # noqa: E402  (the batch and the streaming-read line)


def bench(reads, read_samples, k, reps, stream_tbps, text):
    import torch
    from poregen_amd.engine import EventAligner, ModelFit
    rng = np.random.default_rng(k)
    levels = rng.integers(60000, 130000, 4 ** k).astype(np.uint32)
    stdvs = rng.integers(1500, 4000, 4 ** k).astype(np.uint32)
    hb = fit_bench.make_batch(np.full(reads, read_samples, np.int64), levels, k)
    db = hb.to_device("cuda:0")
    fit = ModelFit(levels, k)
    fr = fit.submit(db)
    fit.close()
    best, wall, got = None, None, None
    with EventAligner(levels, stdvs, k, text=text) as ea:
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ea.submit(db, fr)
            dt = time.perf_counter() - t0
            ms = ea.kernel_ms()
            if i:
                best = ms if best is None else tuple(min(a, b) for a, b in zip(best, ms)); wall = dt if wall is None else min(wall, dt)
    n_samples, n_ops, n_rows = int(hb.sig_off[-1]), int(hb.op_off[-1]), len(got.rows)
    text_bytes = len(got.text) if got.text else 0
    moved = 2 * n_samples + 5 * n_ops
    stream = stream_tbps * 1e12 if stream_tbps else None
    return dict(shape=f"configs[1]: {reads} x {read_samples}", k=k, text=text, reads=reads, samples=n_samples, ops=n_ops, fitted_reads=int((fr.status == 0).sum()), rows=n_rows,
                text_bytes=text_bytes, count_ms=best[0], rows_ms=best[1], text_ms=best[2] if text else None, submit_ms=wall * 1e3, rows_per_s=n_rows / (best[1] * 1e-3),
                text_bytes_per_s=text_bytes / (best[2] * 1e-3) if text else None, rows_read_bytes=moved, rows_read_bytes_per_s=moved / (best[1] * 1e-3),
                rows_share_of_stream_read=moved / (best[1] * 1e-3) / stream if stream else None,
                text_share_of_stream_read=text_bytes / (best[2] * 1e-3) / stream if stream and text else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-samples", type=int, default=4000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evalign_bench.json"))
    args = ap.parse_args()
    out = {"stream_read_tbps": fit_bench.stream_read_tbps(), "runs": []}
    out["runs"].append(bench(args.reads, args.read_samples, args.k, args.reps, out["stream_read_tbps"], True))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
