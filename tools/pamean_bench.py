#!/usr/bin/env python3
"""pamean_bench.py -- `poregen subtool0` / `pa_stats` (pg_pamean_*) on one MI355X.

Measured, each as the best of --reps runs after one warm-up, with a device synchronise inside the time:
  device   the configs[1]-shaped batch (synth.make_batch_fast: 50 000 reads x 4 000 samples, 400 MB of int16) and the ragged workload
           (synth.ragged_lengths + make_ragged_fast, 200 M samples) already in HBM (torch tensors, PG_LOC_DEVICE): one read_means()
           call on one reused handle = offsets to the host, two kernels, 48 bytes per read back, the host's fallback loop and the summary. Bytes / time and
           the same over the whole call (`call_of_hbm_peak`: not a kernel figure), and the fallback count.
  kernels  --trace DB: the database of a separate `rocprofv3 --kernel-trace --stats` run of `--only device`. Per workload, the median
           time of k_pa_sums and k_pa_final, and the bytes of int16 samples over the sum of the two: the kernels' share of the 8 TB/s
           HBM peak, the figure the targets are set in. --trace-out writes the table as text.
  host     the configs[1] batch in page-locked host memory (PG_LOC_HOST), next to a plain H2D copy of the same bytes.
  cli      bin/poregen subtool0 on an uncompressed BLOW5 and on a zlib + svb-zd BLOW5 of the same --cli-reads reads (files in the page
           cache), with the host-decode / device-wait split the CLI reports on stderr; pa_stats on the uncompressed one. A third file,
           none + svb-zd, holds the same blocks without the record compression: its host-decode time against the zlib file's splits
           the host time into inflate and the rest. --exe LABEL=PATH (repeatable) runs other builds of bin/poregen on the same files,
           the builds taking turns rep by rep (an A/B on one box); every run's time is kept (`runs_s`), so the spread is in the output.
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
PEAK = 8e12


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    best, out = 1e30, None
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best, out


def to_dev(b):
    import torch
    return (torch.from_numpy(b.sig).cuda(), torch.from_numpy(b.sig_off.view(np.int64)).cuda(), torch.from_numpy(b.digitisation).cuda(),
            torch.from_numpy(b.offset).cuda(), torch.from_numpy(b.range).cuda())


def kernel_table(db, workloads, out_path):
    """median k_pa_sums / k_pa_final time per workload from a rocprofv3 database; the workloads are told apart by k_pa_sums' grid
    (one wave per read plus one per extra piece: 50 000 for configs1)"""
    import sqlite3
    import statistics
    rows = sqlite3.connect(db).execute("select name, duration, grid_x / workgroup_x from kernels order by start").fetchall()
    sums = [(d / 1000, g) for n, d, g in rows if "k_pa_sums" in n]
    fin = [d / 1000 for n, d, g in rows if "k_pa_final" in n]
    out, lines = {}, ["kernel times from rocprofv3 --kernel-trace --stats of tools/pamean_bench.py --only device (warm-up + reps launches "
                      "per workload), one MI355X; share = int16 bytes / (k_pa_sums + k_pa_final) / 8 TB/s", ""]
    i = 0
    for name, w in workloads.items():
        grids = sorted({g for _, g in sums}, key=lambda g: abs(g - w["reads"]))
        g = grids[0]
        t = [d for d, gg in sums if gg == g]
        k = len(t)
        f = fin[i:i + k]
        i += k
        ts, tf = statistics.median(t), statistics.median(f)
        out[name] = {"workgroups": g, "launches": k, "k_pa_sums_us": round(ts, 1), "k_pa_sums_min_us": round(min(t), 1),
                     "k_pa_final_us": round(tf, 1), "bytes": w["bytes"], "kernel_GBps": round(w["bytes"] / (ts + tf) / 1e3, 1),
                     "of_hbm_peak": round(w["bytes"] / ((ts + tf) * 1e-6) / PEAK, 3),
                     "k_pa_sums_of_hbm_peak": round(w["bytes"] / (ts * 1e-6) / PEAK, 3)}
        lines.append(f"{name:9s} workgroups {g:6d} launches {k}: k_pa_sums median {ts:7.1f} us (min {min(t):.1f}), k_pa_final {tf:5.1f} us, "
                     f"{out[name]['kernel_GBps']:7.1f} GB/s = {out[name]['of_hbm_peak']:.3f} of peak (k_pa_sums alone {out[name]['k_pa_sums_of_hbm_peak']:.3f})")
    if out_path:
        with open(out_path, "w") as fo:
            fo.write("\n".join(lines) + "\n")
    return out


def device_and_host(a, res, c1, rg, read_means):
    import torch
    res["device"] = {}
    for name, b in (("configs1", c1), ("ragged", rg)):
        d = to_dev(b)
        s, r = timed(lambda: read_means(*d), a.reps)
        nb = b.sig.nbytes
        res["device"][name] = {"reads": b.n_reads, "samples": int(b.sig.size), "bytes": nb, "s": round(s, 6),
                               "call_GBps": round(nb / s / 1e9, 1), "call_of_hbm_peak": round(nb / s / PEAK, 3), "fallback_reads": r.n_fallback,
                               "fallback_share": round(r.n_fallback / b.n_reads, 6), "longest_read": int(np.diff(b.sig_off).max())}
        del d
        torch.cuda.empty_cache()
    if a.only == "device":
        return
    if a.trace:
        res["kernels"] = kernel_table(a.trace, {name: res["device"][name] for name in res["device"]}, a.trace_out)

    pin = [torch.from_numpy(x).pin_memory() for x in (c1.sig, c1.sig_off.view(np.int64), c1.digitisation, c1.offset, c1.range)]
    pin_np = [t.numpy() for t in pin]
    pin_np[1] = pin_np[1].view(np.uint64)
    s_host, _ = timed(lambda: read_means(*pin_np), a.reps)
    dst = torch.empty_like(pin[0], device="cuda")
    s_h2d, _ = timed(lambda: dst.copy_(pin[0], non_blocking=True), a.reps)
    res["host_pinned"] = {"s": round(s_host, 6), "GBps": round(c1.sig.nbytes / s_host / 1e9, 1),
                          "h2d_GBps": round(c1.sig.nbytes / s_h2d / 1e9, 1), "fraction_of_h2d": round(s_h2d / s_host, 3)}
    del pin, pin_np, dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-reads", type=int, default=50000)
    ap.add_argument("--only", choices=["all", "device", "cli"], default="all")
    ap.add_argument("--exe", action="append", default=[], help="LABEL=PATH of another bin/poregen for the cli section")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pamean_bench.json"))
    ap.add_argument("--trace", help="rocprofv3 database of an --only device run")
    ap.add_argument("--trace-out", help="write the kernel table of --trace here")
    a = ap.parse_args()
    import torch
    from poregen_amd import synth
    from poregen_amd.engine import SignalMeans
    if not torch.cuda.is_available():
        raise SystemExit("pamean_bench: no GPU (this tool measures the device path; there is no CPU fallback)")
    sm = SignalMeans()

    def read_means(*arrs):  # one handle for every run: its buffers are allocated once
        sm.submit(*arrs)
        return sm.finish()

    res = {"device_name": torch.cuda.get_device_name(0), "peak_hbm_GBps": PEAK / 1e9}

    c1 = synth.make_batch_fast(50000, 4000, seed=20251003)
    rg = synth.make_ragged_fast(synth.ragged_lengths()) if a.only != "cli" else None
    if a.only != "cli":
        device_and_host(a, res, c1, rg, read_means)
        if a.only == "device":
            print(json.dumps(res))
            return
    sub = c1.slice_reads(0, min(a.cli_reads, c1.n_reads))
    exe = os.path.join(ROOT, "bin", "poregen")
    res["cli"] = {"reads": sub.n_reads, "samples_bytes": int(sub.sig.nbytes)}
    exes = [("", exe)] + [tuple(x.split("=", 1)) for x in a.exe]
    n_runs = max(1, a.reps - 2)
    for kind, comp in (("blow5_none", False), ("blow5_zlib_svbzd", True), ("blow5_none_svbzd", "svb-zd")):
        path = os.path.join(a.tmp, f"pamean_bench_{kind}.blow5")
        synth.write_blow5(sub, path, compress=comp)
        with open(path, "rb") as f:
            while f.read(1 << 26):
                pass
        for cmd in (("subtool0", "pa_stats") if kind == "blow5_none" else ("subtool0",)):
            runs = {label: [] for label, _ in exes}
            for label, e in exes:                                 # one unrecorded run each: the binary and its libraries in the page cache
                subprocess.run([e, cmd, path], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
            for _ in range(n_runs):
                for label, e in exes:
                    t = time.perf_counter()
                    r = subprocess.run([e, cmd, path], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
                    dt = time.perf_counter() - t
                    if r.returncode:
                        raise SystemExit(r.stderr.decode()[-2000:])
                    m = re.search(rb"host decode ([0-9.]+) s, waiting for the device ([0-9.]+) s, total ([0-9.]+) s", r.stderr)
                    runs[label].append((dt, [float(x) for x in m.groups()] if m else None))
            for label, _ in exes:
                best, split = min(runs[label], key=lambda x: x[0])
                res["cli"][f"{cmd}_{kind}" + (f"@{label}" if label else "")] = {
                    "file_bytes": os.path.getsize(path), "s": round(best, 3), "runs_s": [round(x[0], 3) for x in runs[label]],
                    "GBps_of_samples": round(sub.sig.nbytes / best / 1e9, 2),
                    "host_decode_s": split and split[0], "device_wait_s": split and split[1], "in_process_s": split and split[2],
                    "host_decode_runs_s": [x[1] and x[1][0] for x in runs[label]]}
        os.unlink(path)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
