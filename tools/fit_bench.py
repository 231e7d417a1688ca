#!/usr/bin/env python3
"""fit_bench.py -- the two passes of `poregen fit` (pg_fit_submit) on one MI355X.

  The batch is already in HBM (CUDA tensors, PG_LOC_DEVICE) and its signal follows the model, so that every read is fitted and pass 2 sees
  every sample. Per shape -- configs[1] (50 000 reads of 4 000 samples) and a ragged one (lognormal read lengths from 400 to 10^6 samples,
  the same total) -- and per k (5: per-slot sums in LDS; 9: in global memory):
    pass1_ms / pass2_ms   HIP-event time of k_fit_sums / k_fit_resid, the best of --reps submits after one warm-up (pg_fit_pass_ms)
    bytes                 what a pass must read at least once: 2 bytes per sample, 4 per op, 1 per base, the level table (4 * 4^k)
    *_bytes_per_s         those bytes over the pass's time, beside the best plain streaming read of tools/probe/stream_probe.hip in the
                          same run (stream_read_tbps) and the 8 TB/s HBM peak DESIGN.md uses
    *_share_of_stream_read  the same rate over that streaming read: the ratio DESIGN.md section 18.5 quotes
    submit_ms             wall time of the whole call: both passes, the span kernel, the solve on the host and the copies between them
  static: per kernel the registers, scratch, LDS and static instruction counts of tools/isa_stats.py, and the occupancy (waves per SIMD)
  of the compiler's resource remarks (None when hipcc is not there).
Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def stream_read_tbps():
    """the best plain 16-byte streaming read of the probe, TB/s (None when the probe cannot be built or run)"""
    exe = os.path.join(ROOT, "tools", "probe", "stream_probe")
    if not os.path.exists(exe):
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", exe, exe + ".hip"], capture_output=True, text=True)
        if r.returncode:
            return None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    best = [float(m.group(1)) for m in re.finditer(r"^A plain.*?([0-9.]+) TB/s", r.stdout, re.M)]
    return max(best) if best else None


def static_picture():
    """{kernel: vgpr, sgpr, scratch, lds, VALU, SALU, DS, VMEM (tools/isa_stats.py: the allocation, next_free_vgpr), vgprs_used and
    occupancy_waves_per_simd (hipcc -Rpass-analysis=kernel-resource-usage)}"""
    src = os.path.join(ROOT, "poregen_amd", "csrc", "pg_fit.hip")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), src], capture_output=True, text=True, timeout=300)
        rows = [l.split("|") for l in r.stdout.splitlines() if "|" in l and not l.startswith("kernel")]
        c = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-S",
                            "--cuda-device-only", "-o", os.devnull, src], capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired):
        return None
    remarks = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", c.stderr, re.S):
        remarks[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    names = sorted(remarks)   # isa_stats.py prints its rows in the order of the mangled names too
    if r.returncode or c.returncode or len(rows) != len(names) or not names:
        return None
    out = {}
    for name, (left, right) in zip(names, rows):
        short = re.search(r"k_fit_[a-z]+(ILb[01])?", name).group(0).replace("ILb1", "<lds table>").replace("ILb0", "<global table>")
        a, b = [int(x) for x in left.split()[-4:]], [int(x) for x in right.split()]
        out[short] = dict(vgpr=a[0], sgpr=a[1], scratch=a[2], lds=a[3], VALU=b[0], SALU=b[1], DS=b[2], VMEM=b[3], vgprs_used=remarks[name][0],
                          occupancy_waves_per_simd=remarks[name][1])
    return out


def make_batch(read_samples, levels, k, seed=1, chunk=4000):
    """A host Batch whose reads have the given numbers of samples: dwells of 5 to 15 samples, a last op that takes the rest of the read,
    raw = a + b * level + noise for every event that carries a k-mer."""
    from poregen_amd.engine import Batch
    rng = np.random.default_rng(seed)
    n = len(read_samples)
    n_ev = np.maximum((np.asarray(read_samples, np.int64) / 10.6).astype(np.int64) - 10, 1)
    op_off = np.concatenate([[0], np.cumsum(n_ev)]).astype(np.uint64)
    sig_off = np.concatenate([[0], np.cumsum(read_samples)]).astype(np.uint64)
    op_n = rng.integers(5, 16, int(op_off[-1])).astype(np.uint32)
    last = op_off[1:].astype(np.int64) - 1
    body = np.add.reduceat(op_n.astype(np.int64), op_off[:-1].astype(np.int64)) - op_n[last]
    assert np.all(np.asarray(read_samples, np.int64) > body)
    op_n[last] = (np.asarray(read_samples, np.int64) - body).astype(np.uint32)     # the rest of the read: mostly a stall outside --max_dur
    codes = rng.integers(0, 4, int(op_off[-1])).astype(np.int64)
    seq = np.frombuffer(b"ACGT", np.uint8)[codes]
    sig = np.empty(int(sig_off[-1]), np.int16)
    lv = np.asarray(levels, np.float32)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        o0, o1 = int(op_off[lo]), int(op_off[hi])
        c = codes[o0:o1]
        kc = np.zeros(o1 - o0, np.int64)
        for j in range(k):                                                         # the k-mer that starts at every base (wraps at a read's end: only the level is off there)
            kc = kc * 4 + np.roll(c, -j)
        a = np.repeat(rng.uniform(300, 600, hi - lo), n_ev[lo:hi]).astype(np.float32)
        b = np.repeat(rng.uniform(0.004, 0.008, hi - lo), n_ev[lo:hi]).astype(np.float32)
        per_event = a + b * lv[kc]
        s = np.repeat(per_event, op_n[o0:o1].astype(np.int64)) + rng.integers(-12, 13, int(sig_off[hi] - sig_off[lo])).astype(np.float32)
        sig[int(sig_off[lo]):int(sig_off[hi])] = np.rint(s).astype(np.int16)
    return Batch(n_reads=n, sig=sig, sig_off=sig_off, digitisation=np.full(n, 8192.0), offset=np.full(n, 10.0), range=np.full(n, 1400.0),
                 query_start=np.zeros(n, np.int32), target_start=np.zeros(n, np.int32), target_end=n_ev.astype(np.int32), seq=seq.copy(), seq_off=op_off.copy(),
                 op_n=op_n, op_t=np.zeros(op_n.size, np.uint8), op_off=op_off, all_matches=True)


def bench(name, read_samples, k, reps, stream_tbps):
    import torch
    from poregen_amd.engine import ModelFit
    rng = np.random.default_rng(k)
    levels = rng.integers(60000, 130000, 4 ** k).astype(np.uint32)
    hb = make_batch(read_samples, levels, k)
    db = hb.to_device("cuda:0")
    fit = ModelFit(levels, k)
    p1 = p2 = wall = None
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fit.submit(db)
        dt = time.perf_counter() - t0
        a, b = fit.pass_ms()
        if i:
            p1 = a if p1 is None else min(p1, a); p2 = b if p2 is None else min(p2, b); wall = dt if wall is None else min(wall, dt)
    res = fit.finish()
    fit.close()
    n_samples, n_ops = int(hb.sig_off[-1]), int(hb.op_off[-1])
    moved = 2 * n_samples + 4 * n_ops + n_ops + 4 * 4 ** k
    fitted = int((r.status == 0).sum())
    stream = stream_tbps * 1e12 if stream_tbps else None
    return dict(shape=name, k=k, reads=len(read_samples), samples=n_samples, ops=n_ops, fitted_reads=fitted, counted_samples_per_submit=res.samples // (reps + 1),
                bytes=moved, pass1_ms=p1, pass2_ms=p2, submit_ms=wall * 1e3, pass1_bytes_per_s=moved / (p1 * 1e-3), pass2_bytes_per_s=moved / (p2 * 1e-3),
                pass1_share_of_stream_read=moved / (p1 * 1e-3) / stream if stream else None, pass2_share_of_stream_read=moved / (p2 * 1e-3) / stream if stream else None,
                pass1_share_of_hbm_peak=moved / (p1 * 1e-3) / HBM_PEAK, pass2_share_of_hbm_peak=moved / (p2 * 1e-3) / HBM_PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-samples", type=int, default=4000)
    ap.add_argument("--ks", default="5,9")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    total = args.reads * args.read_samples
    rng = np.random.default_rng(3)
    ragged = np.clip(rng.lognormal(8.3, 1.2, 4 * args.reads), 400, 1000000).astype(np.int64)
    ragged = ragged[:int(np.searchsorted(np.cumsum(ragged), total)) + 1]
    out = {"stream_read_tbps": stream_read_tbps(), "static": static_picture(), "runs": []}
    for k in (int(x) for x in args.ks.split(",")):
        out["runs"].append(bench(f"configs[1]: {args.reads} x {args.read_samples}", np.full(args.reads, args.read_samples, np.int64), k, args.reps, out["stream_read_tbps"]))
        out["runs"].append(bench("ragged 400..1000000", ragged, k, args.reps, out["stream_read_tbps"]))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
