#!/usr/bin/env python3
"""pool_bench.py -- `poregen model --pool` and `poregen offsets` end to end on one MI355X, and what the selection costs.

The two dump directories of tools/model_bench.py (k = 5 at sample_limit 5000; k = 9, 262 144 files, most of them empty), written by
`poregen gmove` from seeded synthetic reads. Measured per directory:
  pool START:LEN   bin/poregen model --pool START:LEN DIR -o /dev/null: best wall time of --reps runs, the stages the command prints, and
                   select_ms, the HIP-event time of the seven histogram passes (k_pool_hist + k_pool_pick), hence their bytes/s -- seven
                   reads of 8 bytes per arena value -- beside the best plain streaming-read line of tools/probe/stream_probe.hip
  offsets          the same for bin/poregen offsets DIR (K labelings over one arena)
  concatenated     for the pools only: `poregen model` (--model-bin: the parent commit's binary; by default this build's, whose plain
                   `model` is unchanged) on a directory that holds one file per group, the members' bytes back to back. A file of more
                   than 2^23 values goes to that command's host path there.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
EXE = os.path.join(ROOT, "bin", "poregen")


def timed(cmd, reps, tag):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        wall = time.perf_counter() - t
        if r.returncode:
            raise SystemExit(r.stderr[-2000:])
        if best is None or wall < best["wall_s"]:
            best = {"wall_s": round(wall, 4), "stages": [ln[len(tag):] for ln in r.stderr.splitlines() if ln.startswith(tag)]}
    text = " ".join(best["stages"])
    for key, pat in (("select_ms", r"select_ms: ([0-9.]+)"), ("n_values", r"n_values: (\d+)"), ("n_host_files", r"n_host_files: (\d+)"),
                     ("reading_files_s", r"reading files ([0-9.]+) s")):
        m = re.search(pat, text)
        if m:
            best[key] = float(m.group(1)) if "." in m.group(1) else int(m.group(1))
    if best.get("select_ms") and best.get("n_values"):
        best["select_GBps"] = round(7 * 8 * best["n_values"] / (best["select_ms"] * 1e-3) / 1e9, 2)
    return best


def concatenate(d, out, start, length):
    os.makedirs(out)
    for n in sorted(os.listdir(d), key=lambda x: x.encode()):
        with open(os.path.join(d, n), "rb") as src, open(os.path.join(out, n[start:start + length]), "ab") as dst:
            shutil.copyfileobj(src, dst)
    return out


def measure(d, tmp, name, pools, reps, model_bin):
    res = {"files": len(os.listdir(d)), "bytes": sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d))}
    for start, length in pools:
        key = "pool_%d_%d" % (start, length)
        res[key] = timed([EXE, "model", "--pool", "%d:%d" % (start, length), d, "-o", os.path.join(tmp, "pool_out")], reps, "[model] ")
        cat = concatenate(d, os.path.join(tmp, "%s_cat_%d_%d" % (name, start, length)), start, length)
        res[key]["concatenated"] = timed([model_bin, "model", cat, "-o", os.path.join(tmp, "cat_out")], reps, "[model] ")
        res[key]["equals_concatenated"] = open(os.path.join(tmp, "pool_out")).read() == open(os.path.join(tmp, "cat_out")).read()
        shutil.rmtree(cat, ignore_errors=True)
    res["offsets"] = timed([EXE, "offsets", d, "-o", os.path.join(tmp, "offsets_out")], reps, "[offsets] ")
    res["offsets"]["best"] = [ln for ln in open(os.path.join(tmp, "offsets_out")).read().splitlines() if ln.startswith("best")]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--k9-reads", type=int, default=20000)
    ap.add_argument("--k9-limit", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--model-bin", default=EXE, help="the binary whose plain `model` reads the concatenated directories (the parent commit's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench: no GPU (this tool measures the device path; there is no CPU fallback)")
    import model_bench
    res = {"device_name": torch.cuda.get_device_name(0), "stream_read_TBps": model_bench.stream_read_tbps()}
    tmp = tempfile.mkdtemp(prefix="pg_pool_bench_", dir=a.tmp)
    try:
        d5, _, s5 = model_bench.write_dump(tmp, "k5", "rna004", a.reads, 5, 5000, ["--rna", "--min_dur", "20", "--max_dur", "40"])
        res["k5"] = dict(measure(d5, tmp, "k5", [(0, 1), (2, 1), (1, 3)], a.reps, a.model_bin), gmove_s=round(s5, 2), reads=a.reads, sample_limit=5000)
        d9, _, s9 = model_bench.write_dump(tmp, "k9", "dna_r10", a.k9_reads, 9, a.k9_limit, [])
        res["k9"] = dict(measure(d9, tmp, "k9", [(0, 1), (2, 5), (2, 6)], a.reps, a.model_bin), gmove_s=round(s9, 2), reads=a.k9_reads, sample_limit=a.k9_limit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
