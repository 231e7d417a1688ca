#!/usr/bin/env python3
"""Throughput of `poregen f1_score` (pg_fscore_*). Workload: seeded ragged alignment pairs (synth.alignment_pairs over
synth.ragged_lengths) holding about --gb GB of ss bytes. Prints one JSON line (and writes it to --out):
  device   : ss resident on the device (CUDA tensor), submit + finish, GB/s of ss bytes and the share of 8 TB/s
  pinned   : ss in page-locked host memory
  cli_bam  : `poregen f1_score` end to end on BAM files of the first --cli-gb GB, at --read_limit 0 and at the default (100)
  numpy    : tests/f1_ref.py's per-point restatement on one core, on the first --ref-mb MB (extrapolated as GB/s)
--device-only runs the device pass alone (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from poregen_amd import synth  # noqa: E402
from poregen_amd.engine import AlignmentScorer  # noqa: E402


def workload(gb, seed):
    # about 0.27 ss bytes per signal point per side at the generator's default dwell
    L = synth.ragged_lengths(int(gb * 1.85e9), seed=seed, lo=2000, hi=200_000, median=12_000)
    pairs = synth.alignment_pairs(L, seed=seed)
    parts, off, sig, ref = [], [0], [], []
    n = 0
    for _, ss1, si1, ss2, si2 in pairs:
        for s, si in ((ss1, si1), (ss2, si2)):
            parts.append(s)
            n += len(s)
            off.append(n)
            v = si.split(",")
            sig.append(int(v[0])); ref.append(int(v[2]))
    ss = np.frombuffer(bytearray(b"".join(parts)), np.uint8)  # writable: torch.from_numpy shares it
    return pairs, ss, np.array(off, np.uint64), np.array(sig, np.int64), np.array(ref, np.int64)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--cli-gb", type=float, default=0.25)
    ap.add_argument("--ref-mb", type=float, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    t0 = time.perf_counter()
    pairs, ss, off, sig, ref = workload(a.gb, a.seed)
    res = dict(metric="f1_score", ss_bytes=int(ss.size), pairs=len(pairs), gen_s=round(time.perf_counter() - t0, 1))
    sc = AlignmentScorer(threshold=1)

    def run(x):
        sc.submit(x, off, sig, ref)
        return sc.finish()
    dev = torch.from_numpy(ss).cuda()
    t, got = timed(lambda: run(dev), a.reps)
    res["device_s"] = round(t, 4)
    res["device_GBps"] = round(ss.size / t / 1e9, 1)
    res["device_share_of_8TBps"] = round(ss.size / t / 8e12, 4)
    res["totals"] = [int(v) for v in got.totals]
    if not a.device_only:
        pin = torch.from_numpy(ss).pin_memory()
        t, got2 = timed(lambda: run(pin.numpy()), a.reps)
        assert np.array_equal(got2.totals, got.totals)
        res["pinned_s"] = round(t, 4)
        res["pinned_GBps"] = round(ss.size / t / 1e9, 1)
        # numpy restatement on one core
        import f1_ref as R
        k, nb = 0, 0
        t0 = time.perf_counter()
        while k < len(pairs) and nb < a.ref_mb * 1e6:
            _, s1, i1, s2, i2 = pairs[k]
            R.pair_counts(s1, i1, s2, i2, threshold=1)
            nb += len(s1) + len(s2)
            k += 1
        t = time.perf_counter() - t0
        res["numpy_ref_GBps"] = round(nb / t / 1e9, 4)
        res["numpy_ref_bytes"] = nb
        # CLI end to end on BAM
        with tempfile.TemporaryDirectory(prefix="f1b") as tmp:
            m = int(np.searchsorted(off[2::2], a.cli_gb * 1e9)) + 1
            m = min(m, len(pairs))
            p1, p2 = os.path.join(tmp, "1.bam"), os.path.join(tmp, "2.bam")
            synth.write_alignment_bam(p1, [dict(name=p[0], ss=p[1], si=p[2]) for p in pairs[:m]])
            synth.write_alignment_bam(p2, [dict(name=p[0], ss=p[3], si=p[4]) for p in pairs[:m]])
            res["cli_pairs"] = m
            res["cli_ss_bytes"] = int(off[2 * m])
            res["cli_bam_bytes"] = os.path.getsize(p1) + os.path.getsize(p2)
            for lim in ("0", "100"):
                best = 1e9
                for _ in range(3):
                    t0 = time.perf_counter()
                    r = subprocess.run([os.path.join(ROOT, "bin", "poregen"), "f1_score", p1, p2, "--threshold", "1", "--read_limit", lim],
                                       capture_output=True, timeout=600)
                    best = min(best, time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr
                res[f"cli_limit{lim}_s"] = round(best, 3)
            res["cli_limit0_GBps"] = round(res["cli_ss_bytes"] / res["cli_limit0_s"] / 1e9, 2)
    sc.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
