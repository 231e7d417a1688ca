#!/usr/bin/env python3
"""model_bench.py -- `poregen model` end to end on one MI355X, and what bounds it.

Two dump directories are written by `poregen gmove` from seeded synthetic reads (both in the page cache afterwards):
  k5    the reads of BASELINE configs[2]'s per-GPU shard (--reads RNA004 reads, k = 5, sample_limit 5000): 1024 files
  k9    DNA reads, k = 9, a small sample_limit: 262 144 files, most of them empty
Measured per directory:
  cli        bin/poregen model DIR -o /dev/null --dwell_model /dev/null: best wall time of --reps runs, with the stages the command
             prints (listing, device context, reading files, submit, finish, printing)
  device     the same files through engine.DumpModel(profile=True) from bytes already in host memory: HIP-event time of the parse
             kernels (k_dt_count .. k_dt_evlen) and of the reduction, parse bytes/s, next to the plain streaming-read figure
             of tools/probe/stream_probe.hip on the same machine (its best "A plain" line)
  events     the same batches through DumpModel(profile=True, events=True): event_ms, the HIP-event time of k_ev_stats + k_ev_carry
             (pg_evstat.hip) over the parsed values, next to parse_ms and model_ms of the same run; the 8 bytes per value it reads as
             GB/s and as a fraction of the streaming-read figure; reduce_ms, the two reductions over one value per event behind it
  cpu        oracle/model_oracle stats + dwell over the same directory on one core (the pipeline's tr | tail | datamash restated in C)
Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "bin", "poregen")
ORACLE = os.path.join(ROOT, "oracle", "model_oracle")


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


def write_dump(tmp, name, kind, reads, k, limit, extra):
    from poregen_amd import synth
    b = synth.make_batch_fast(reads, kind=kind, seed=2026)
    pre = os.path.join(tmp, name + "_in")
    synth.write_blow5(b, pre + ".blow5"); synth.write_paf_fastq(b, pre)
    out = os.path.join(tmp, name)
    cmd = [EXE, "gmove", "-k", str(k), "--scaling", "1", "--file_limit", str(4 ** k), "--sample_limit", str(limit), pre + ".blow5", pre + ".paf",
           "--fastq", pre + ".fastq", out, "--raw_model", os.path.join(tmp, name + "_raw")] + extra
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode:
        raise SystemExit(r.stderr[-2000:])
    return os.path.join(out, "dump"), os.path.join(tmp, name + "_raw"), time.perf_counter() - t


def measure(d, raw, reps):
    from poregen_amd.engine import DumpModel, list_dump_dirs
    names, paths = list_dump_dirs([d])
    blobs = [open(p[0], "rb").read() for p in paths]         # (also: the page cache)
    n_bytes = sum(len(x) for x in blobs)
    res = {"files": len(names), "bytes": n_bytes}
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        r = subprocess.run([EXE, "model", d, "-o", os.path.join(os.path.dirname(raw), "model_out"), "--dwell_model", "/dev/null"], capture_output=True, text=True, timeout=120)
        wall = time.perf_counter() - t
        if r.returncode:
            raise SystemExit(r.stderr[-2000:])
        if best is None or wall < best["wall_s"]:
            best = {"wall_s": round(wall, 4), "stages": [ln[len("[model] "):] for ln in r.stderr.splitlines() if ln.startswith("[model] ")]}
    best["equals_gmove_raw_model"] = open(os.path.join(os.path.dirname(raw), "model_out")).read() == open(raw).read()
    m = re.search(r"reading files ([0-9.]+) s", " ".join(best["stages"]))
    best["reading_files_s"] = float(m.group(1)) if m else None
    res["cli"] = best
    # the device alone: bytes in host memory, batches as the command cuts them
    off, batches, cur = [0], [], []
    for x in blobs:
        if cur and off[-1] + len(x) > (64 << 20):
            batches.append((b"".join(cur), off)); off, cur = [0], []
        cur.append(x); off.append(off[-1] + len(x))
    batches.append((b"".join(cur), off))
    dm = DumpModel(profile=True)
    best = None
    for _ in range(reps + 1):
        t = time.perf_counter()
        for data, o in batches:
            dm.submit(data, o)
        _, info = dm.finish()
        wall = time.perf_counter() - t
        if best is None or info.parse_ms < best["parse_ms"]:
            best = {"wall_s": round(wall, 4), "parse_ms": round(info.parse_ms, 4), "model_ms": round(info.model_ms, 4), "n_values": info.n_values,
                    "n_host_files": info.n_host_files, "n_batches": info.n_batches,
                    "parse_GBps": round(n_bytes / (info.parse_ms * 1e-3) / 1e9, 2) if info.parse_ms else None}
    dm.close()
    res["device"] = best
    dm = DumpModel(profile=True, events=True)
    best = None
    for _ in range(reps + 1):
        for data, o in batches:
            dm.submit(data, o)
        _, info = dm.finish()
        ev = dm.finish_events()
        if best is None or ev.event_ms < best["event_ms"]:
            best = {"event_ms": round(ev.event_ms, 4), "reduce_ms": round(ev.reduce_ms, 4), "parse_ms": round(info.parse_ms, 4), "model_ms": round(info.model_ms, 4),
                    "n_values": info.n_values, "n_events": int(ev.n_events.sum()), "n_refused": int((ev.status != 0).sum()),
                    "event_GBps": round(info.n_values * 8 / (ev.event_ms * 1e-3) / 1e9, 2) if ev.event_ms else None}
    dm.close()
    res["events"] = best
    t = time.perf_counter()
    for mode in (["stats", d, "3.1"], ["dwell", d]):
        subprocess.run([ORACLE] + mode, stdout=subprocess.DEVNULL, check=True)
    res["cpu_model_oracle_1core_s"] = round(time.perf_counter() - t, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--k9-reads", type=int, default=20000)
    ap.add_argument("--k9-limit", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("model_bench: no GPU (this tool measures the device path; there is no CPU fallback)")
    res = {"device_name": torch.cuda.get_device_name(0), "stream_read_TBps": stream_read_tbps()}
    tmp = tempfile.mkdtemp(prefix="pg_model_bench_", dir=a.tmp)
    try:
        d5, raw5, s5 = write_dump(tmp, "k5", "rna004", a.reads, 5, 5000, ["--rna", "--min_dur", "20", "--max_dur", "40"])
        res["k5"] = dict(measure(d5, raw5, a.reps), gmove_s=round(s5, 2), reads=a.reads, sample_limit=5000)
        d9, raw9, s9 = write_dump(tmp, "k9", "dna_r10", a.k9_reads, 9, a.k9_limit, [])
        res["k9"] = dict(measure(d9, raw9, a.reps), gmove_s=round(s9, 2), reads=a.k9_reads, sample_limit=a.k9_limit)
        for k in ("k5", "k9"):   # the new kernel against the plain streaming read of the same machine
            gbps = res[k]["events"]["event_GBps"]
            res[k]["events"]["fraction_of_stream_read"] = round(gbps / (res["stream_read_TBps"] * 1e3), 4) if gbps and res["stream_read_TBps"] else None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
