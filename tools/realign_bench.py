#!/usr/bin/env python3
"""realign_bench.py -- the alignment kernel of `poregen realign` (pg_realign_submit) beside the two passes of `poregen fit` on one MI355X.

  The batches are those of tools/fit_bench.py: already in HBM (PG_LOC_DEVICE), the signal following the model so that every read is
  fitted and every boundary between two counted events is free. Per shape -- configs[1] (50 000 reads of 4 000 samples) and the ragged
  one -- and per k (5 and 9), from ONE run:
    pass1_ms / pass2_ms   HIP-event time of fit's k_fit_sums / k_fit_resid on the batch (pg_fit_pass_ms), the best of --reps after a warm-up
    align_ms              HIP-event time of k_rl_align (pg_realign_kernel_ms), likewise; per band in --bands
    free / moved          boundaries the kernel could move and did
    ns_per_free_boundary  align_ms over the free boundaries
    bytes                 what the kernel must read at least once (2 bytes per sample, 4 per op, 1 per base, the level table) and write (4 per
                          op); align_share_of_stream_read: those bytes over align_ms beside the best plain streaming read of
                          tools/probe/stream_probe.hip in the same run
    submit_c_ms           wall time of the library's pg_realign_submit alone; submit_ms is Realigner.submit, which also clones the ops and
                          turns 2 x 128 bits per read into Python ints
    submit_ms             wall time of the whole Realigner.submit: the span and starts kernels, the one wait between them and the alignment,
                          the alignment, the per-read reduction and the copy of 48 bytes per read
    align_ms_reps / submit_ms_reps   every repetition behind the warm-up: their spread is the margin of an A/B (--lib) on the same box
    rounds_ms             with --rounds R > 1: wall time of R rounds of pg_fit_submit + pg_realign_submit on one pair of handles, the phase
                          alternating between 0 and 128, every round's ops the next one's input
  --phase sets the pinned period's phase of the timed submits; --lib loads another build of libpgmove.so (one from before the phase
  takes phase 0 only).
  static: per kernel the registers, scratch, LDS and static instruction counts of tools/isa_stats.py and the occupancy of the compiler's
  resource remarks (None when hipcc is not there).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fit_bench import make_batch, stream_read_tbps  # noqa: E402


def static_picture():
    src = os.path.join(ROOT, "poregen_amd", "csrc", "pg_realign.hip")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), src], capture_output=True, text=True, timeout=300)
        rows = [l.split("|") for l in r.stdout.splitlines() if "|" in l and not l.startswith("kernel")]
        c = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-S",
                            "--cuda-device-only", "-o", os.devnull, src], capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired):
        return None
    remarks = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", c.stderr, re.S):
        remarks[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    names = sorted(remarks)   # isa_stats.py prints its rows in the order of the mangled names too
    if r.returncode or c.returncode or len(rows) != len(names) or not names:
        return None
    out = {}
    for name, (left, right) in zip(names, rows):
        a, b = [int(x) for x in left.split()[-4:]], [int(x) for x in right.split()]
        out[re.search(r"k_rl_[a-z]+", name).group(0)] = dict(vgpr=a[0], sgpr=a[1], scratch=a[2], lds=a[3], VALU=b[0], SALU=b[1], DS=b[2], VMEM=b[3], vgprs_used=remarks[name][0],
                                                             occupancy_waves_per_simd=remarks[name][1], lds_bytes_per_block=remarks[name][2])
    return out


def bench(name, read_samples, k, bands, reps, stream_tbps, phase=0, rounds=1):
    import torch
    import ctypes as C
    from poregen_amd import _abi, engine
    from poregen_amd.engine import ModelFit, Realigner
    rng = np.random.default_rng(k)
    levels = rng.integers(60000, 130000, 4 ** k).astype(np.uint32)
    hb = make_batch(read_samples, levels, k)
    db = hb.to_device("cuda:0")
    fit = ModelFit(levels, k)
    p1 = p2 = None
    for i in range(reps + 1):
        fr = fit.submit(db)
        a, b = fit.pass_ms()
        if i:
            p1 = a if p1 is None else min(p1, a); p2 = b if p2 is None else min(p2, b)
    fit.finish()
    fit.close()
    n_samples, n_ops = int(hb.sig_off[-1]), int(hb.op_off[-1])
    moved_bytes = 2 * n_samples + 4 * n_ops + n_ops + 4 * 4 ** k + 4 * n_ops
    stream = stream_tbps * 1e12 if stream_tbps else None
    out = dict(shape=name, k=k, reads=len(read_samples), samples=n_samples, ops=n_ops, pieces=int(np.sum((np.diff(hb.op_off.astype(np.int64)) + 255) // 256)),
               fitted_reads=int((fr.status == 0).sum()), bytes=moved_bytes, pass1_ms=p1, pass2_ms=p2, bands=[])
    for band in bands:
        ra = Realigner(levels, k, band=band, phase=phase)
        all_ms, all_wall = [], []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = ra.submit(db, fr)
            dt = time.perf_counter() - t0
            t = ra.kernel_ms()
            if i:
                all_ms.append(t); all_wall.append(dt * 1e3)
        ms, wall = min(all_ms), min(all_wall) * 1e-3
        # the library call alone, without what the Python layer does with its result (the clone of the ops, 128-bit costs as Python ints)
        cb = engine._c_batch(db)
        st_, a_, b_ = (np.ascontiguousarray(x, dtype=t) for x, t in ((fr.status, np.uint32), (fr.a, np.float64), (fr.b, np.float64)))
        res = _abi.PgRealignReads()
        all_c = []
        for i in range(reps + 1):
            res.struct_size = C.sizeof(_abi.PgRealignReads)
            t0 = time.perf_counter()
            rc = ra._lib.pg_realign_submit(ra._h, C.byref(cb), st_.ctypes.data, a_.ctypes.data, b_.ctypes.data, C.byref(res))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0
            ra.kernel_ms()
            if i:
                all_c.append(dt)
        rounds_ms = None
        if rounds > 1:
            import copy
            fit2 = ModelFit(levels, k)
            for i in range(reps + 1):
                b = copy.copy(db)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(1, rounds + 1):
                    f = fit2.submit(b)
                    ra.set_phase(0 if t % 2 else 128)
                    b.op_n = ra.submit(b, f, copy=False).op_n
                dt = (time.perf_counter() - t0) * 1e3
                fit2.finish()
                if i:
                    rounds_ms = dt if rounds_ms is None else min(rounds_ms, dt)
            fit2.close()
        ra.close()
        free, n_moved = int(r.n_free.sum()), int(r.n_moved.sum())
        before, after = sum(r.cost_before), sum(r.cost_after)
        out["bands"].append(dict(band=band, min_len=3, phase=phase, align_ms=ms, submit_ms=wall * 1e3, align_ms_reps=all_ms, submit_ms_reps=all_wall, submit_c_ms=min(all_c), submit_c_ms_reps=all_c, rounds=rounds, rounds_ms=rounds_ms, free=free, moved=n_moved, ns_per_free_boundary=ms * 1e6 / max(free, 1),
                                 align_over_pass2=ms / p2, align_bytes_per_s=moved_bytes / (ms * 1e-3), align_share_of_stream_read=moved_bytes / (ms * 1e-3) / stream if stream else None,
                                 cost_after_over_before=after / before if before else None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-samples", type=int, default=4000)
    ap.add_argument("--ks", default="5,9")
    ap.add_argument("--bands", default="10,31")
    ap.add_argument("--out", default=None)
    ap.add_argument("--phase", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-static", action="store_true")
    args = ap.parse_args()
    if args.lib:
        from poregen_amd import _abi
        _abi.LIB_PATH = os.path.abspath(args.lib)
    total = args.reads * args.read_samples
    rng = np.random.default_rng(3)
    ragged = np.clip(rng.lognormal(8.3, 1.2, 4 * args.reads), 400, 1000000).astype(np.int64)
    ragged = ragged[:int(np.searchsorted(np.cumsum(ragged), total)) + 1]
    bands = [int(x) for x in args.bands.split(",")]
    out = {"stream_read_tbps": stream_read_tbps(), "static": None if args.no_static else static_picture(), "lib": args.lib, "runs": []}
    for k in (int(x) for x in args.ks.split(",")):
        out["runs"].append(bench(f"configs[1]: {args.reads} x {args.read_samples}", np.full(args.reads, args.read_samples, np.int64), k, bands, args.reps, out["stream_read_tbps"], args.phase, args.rounds))
        out["runs"].append(bench("ragged 400..1000000", ragged, k, bands, args.reps, out["stream_read_tbps"], args.phase, args.rounds))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
