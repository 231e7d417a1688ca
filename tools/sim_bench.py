#!/usr/bin/env python3
"""sim_bench.py -- the two kernels of `poregen simulate` (pg_sim_generate) on one MI355X.

  The sequences are already in HBM (CUDA tensors, PG_LOC_DEVICE). Per shape -- the one of tools/fit_bench.py's configs[1] (50 000 reads of
  400 bases: 4 000 samples each at the mean dwell of 10) and its ragged one (lognormal read lengths, the same total) -- and per k (5 and 9):
    ops_ms / emit_ms        HIP-event time of k_sim_ops / k_sim_emit, the best of --reps generates after one warm-up (pg_sim_kernel_ms)
    emit_bytes              what k_sim_emit writes: 2 bytes per sample and 4 per op
    emit_bytes_per_s        those bytes over emit_ms, beside the best plain 16-byte streaming WRITE of tools/probe/stream_probe.hip in the
                            same run (stream_write_tbps) -- emit_share_of_stream_write is the ratio
    emit_samples_per_s      samples (one Philox4x32-10 block each) per second
    generate_ms             wall time of the whole call: both kernels, the scan on the host and the copies between them
    ideal_emit_ms           the same shape with every stdv 0 (no Philox block per sample): what the store path alone costs
  static: per kernel the registers, scratch, LDS and static instruction counts of tools/isa_stats.py.
  --lib PATH measures another build of the library (make variant NAME=lane16 EXTRA=-DPG_SIM_LANE=16).
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


def stream_write_tbps():
    """the best plain 16-byte streaming write of the probe, TB/s (None when the probe cannot be built or run)"""
    exe = os.path.join(ROOT, "tools", "probe", "stream_probe")
    if not os.path.exists(exe):
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", exe, exe + ".hip"], capture_output=True, text=True)
        if r.returncode:
            return None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, PROBE_ONLY_WRITE="1"))
    best = [float(m.group(1)) for m in re.finditer(r"^W plain.*?([0-9.]+) TB/s", r.stdout, re.M)]
    return max(best) if best else None


def static_picture():
    src = os.path.join(ROOT, "poregen_amd", "csrc", "pg_sim.hip")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), src], capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired):
        return None
    rows = [l.split("|") for l in r.stdout.splitlines() if "|" in l and not l.startswith("kernel")]
    if r.returncode or len(rows) != 2:
        return None
    out = {}
    for name, (left, right) in zip(("k_sim_emit", "k_sim_ops"), rows):   # isa_stats.py prints its rows in the order of the mangled names
        a, b = [int(x) for x in left.split()[-4:]], [int(x) for x in right.split()]
        out[name] = dict(vgpr=a[0], sgpr=a[1], scratch=a[2], lds=a[3], VALU=b[0], SALU=b[1], DS=b[2], VMEM=b[3])
    return out


def bench(name, read_bases, k, reps, write_tbps):
    import torch
    from poregen_amd.engine import SignalSimulator
    rng = np.random.default_rng(k)
    n = 4 ** k
    levels, stdvs, dwells = rng.integers(60000, 130000, n).astype(np.uint32), rng.integers(1000, 3000, n).astype(np.uint32), np.full(n, 10, np.uint32)
    seq_off = np.concatenate([[0], np.cumsum(read_bases)]).astype(np.int64)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(seq_off[-1]))]
    d_seq, d_off = torch.from_numpy(seq.copy()).cuda(), torch.from_numpy(seq_off).cuda()
    res = {}
    for label, sd in (("", stdvs), ("ideal_", np.zeros(n, np.uint32))):
        sim = SignalSimulator(levels, sd, dwells, k, seed=1, spread_pct=50, off_spread=10, lead=0)
        ops = emit = wall = None
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = sim.generate(seq=d_seq, seq_off=d_off)
            dt = time.perf_counter() - t0
            a, b = sim.kernel_ms()
            if i:
                ops = a if ops is None else min(ops, a); emit = b if emit is None else min(emit, b); wall = dt if wall is None else min(wall, dt)
        res[label] = (ops, emit, wall, r.n_samples, r.n_ops, r.n_refused)
        sim.close()
    ops, emit, wall, n_samples, n_ops, n_refused = res[""]
    moved = 2 * n_samples + 4 * n_ops
    stream = write_tbps * 1e12 if write_tbps else None
    return dict(shape=name, k=k, reads=len(read_bases), samples=n_samples, ops=n_ops, refused=n_refused, ops_ms=ops, emit_ms=emit, generate_ms=wall * 1e3, emit_bytes=moved,
                emit_bytes_per_s=moved / (emit * 1e-3), emit_samples_per_s=n_samples / (emit * 1e-3), emit_share_of_stream_write=moved / (emit * 1e-3) / stream if stream else None,
                ideal_emit_ms=res["ideal_"][1], ideal_emit_bytes_per_s=moved / (res["ideal_"][1] * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-bases", type=int, default=400)
    ap.add_argument("--ks", default="5,9")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lib:
        from poregen_amd import _abi
        _abi.LIB_PATH = os.path.abspath(args.lib)
    total = args.reads * args.read_bases
    rng = np.random.default_rng(3)
    ragged = np.clip(rng.lognormal(8.3, 1.2, 4 * args.reads) / 10, 40, 100000).astype(np.int64)
    ragged = ragged[:int(np.searchsorted(np.cumsum(ragged), total)) + 1]
    out = {"lib": args.lib, "stream_write_tbps": stream_write_tbps(), "static": None if args.lib else static_picture(), "runs": []}
    for k in (int(x) for x in args.ks.split(",")):
        out["runs"].append(bench(f"configs[1]: {args.reads} x {args.read_bases} bases", np.full(args.reads, args.read_bases, np.int64), k, args.reps, out["stream_write_tbps"]))
        out["runs"].append(bench("ragged 40..100000 bases", ragged, k, args.reps, out["stream_write_tbps"]))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
