#!/usr/bin/env python3
"""scale_bench.py -- what `gmove --reform --scale_model` adds to a batch, on one MI355X.

  device   20 000 reads of 4 000 samples (tools/mvops_bench.py's command-line workload) as a device batch, a random 5-mer model: the wall
           time of ModelFit.calibrate beside ModelFit.submit of the same batch (best of --reps after a warm-up), the HIP-event time of
           k_fit_solve + k_fit_tally inside the calibration, and the HIP-event time of k_scale_records in a profiled scaling-2 collector.
  cli      wall time, median of --runs, of `gmove --reform` with and without --scale_model on the same files.
Prints one JSON object and writes it to --out. One box, one run: no threshold hangs on these numbers.
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


def bench_device(n_reads, reps):
    import torch
    from poregen_amd import synth
    from poregen_amd.engine import GmoveEngine, GmoveParams, ModelFit, generate_kmers
    b = synth.make_batch_fast(n_reads, kind="dna_r10", seed=11)
    b.all_matches = True
    d = b.to_device("cuda:0")
    levels = np.random.default_rng(1).integers(60000, 130000, 1024).astype(np.uint32)
    fit = ModelFit(levels, 5)
    best = dict(calibrate_wall_ms=None, submit_wall_ms=None, solve_event_ms=None)
    for i in range(reps + 1):
        for key, fn in (("calibrate_wall_ms", lambda: fit.calibrate(d)), ("submit_wall_ms", lambda: fit.submit(d))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            ms = (time.perf_counter() - t0) * 1e3
            if i:
                best[key] = min(ms, best[key] or ms)
                if key == "calibrate_wall_ms":
                    best["solve_event_ms"] = min(r.solve_ms, best["solve_event_ms"] or r.solve_ms)
        fit.finish()
    sc = fit.calibrate(d)
    eng = GmoveEngine(GmoveParams(kmers=generate_kmers(5), kmer_size=5, scaling=2, sample_limit=100, profile=True))
    for _ in range(reps + 1):
        eng.submit(d, scaling=sc)
        eng.sync()
    st = eng.kernel_stats()
    eng.close(); fit.close()
    launches, total = st.get("k_scale_records", (0, 0.0))
    return dict(reads=n_reads, samples=int(b.sig_off[-1]), ops=int(b.op_off[-1]), used=sc.n_ok, per_status=sc.n_status, reps=reps,
                k_scale_records_event_ms=(total / launches if launches else None), **best)


def bench_cli(n_reads, runs, tmp):
    from poregen_amd import synth
    b = synth.make_batch_fast(n_reads, kind="dna_r10", seed=11)
    b.target_start = np.zeros_like(b.target_start)
    pre = os.path.join(tmp, "sm")
    synth.write_bam(b, pre + ".bam", block_bytes=60000)
    synth.write_blow5(b, pre + ".blow5")
    levels = np.random.default_rng(1).integers(60000, 130000, 1024)
    names = [""]
    for _ in range(5):
        names = [p + c for p in names for c in "ACGT"]
    with open(pre + ".model", "w") as f:
        f.write("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{levels[i] / 1000:.3f}\t2.000\n" for i, km in enumerate(names)))
    exe = os.path.join(ROOT, "bin", "poregen")
    opts = ["-k", "5", "--file_limit", "1024", "--sample_limit", "1000000", "--index_end", "1023"]   # a slice: every read is read

    def timed(cmd):
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
        return time.perf_counter() - t0

    plain, scaled = [], []
    for i in range(runs + 1):
        for d in ("o1", "o2"):
            shutil.rmtree(os.path.join(tmp, d), ignore_errors=True)
        a = timed([exe, "gmove", "--reform", pre + ".blow5", pre + ".bam"] + opts + [os.path.join(tmp, "o1")])
        s = timed([exe, "gmove", "--reform", "--scale_model", pre + ".model", pre + ".blow5", pre + ".bam"] + opts + [os.path.join(tmp, "o2")])
        if i:
            plain.append(a); scaled.append(s)
    return dict(reads=n_reads, samples=int(b.sig_off[-1]), runs=runs, plain_median_s=statistics.median(plain), scale_model_median_s=statistics.median(scaled),
                plain_s=plain, scale_model_s=scaled)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--cases", default="device,cli")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {}
    if "device" in args.cases.split(","):
        out["device"] = bench_device(args.reads, args.reps)
    if "cli" in args.cases.split(","):
        tmp = tempfile.mkdtemp(prefix="scale_bench", dir=args.tmp)
        try:
            out["cli"] = bench_cli(args.reads, args.runs, tmp)
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
