#!/usr/bin/env python3
"""sigenc_bench.py -- the svb-zd encoder (pg_sigenc_*, csrc/pg_svbenc.hip) alone on one MI355X, and `poregen simulate` with and without it.

  The samples are already in HBM (a CUDA tensor, PG_LOC_DEVICE). Per shape -- `simulate`'s configs[1] (50 000 reads x 4 000 samples) and
  the ragged workload of tools/sigdec_bench.py (synth.ragged_lengths, 200 M samples, reads of up to 10^6) --:
    lens_ms / emit_ms     HIP-event time of the sizes kernel and of the emit kernel, the best of --reps encodes after one warm-up
    bytes                 what the two kernels move: 4 bytes read per sample (two passes) plus the block bytes written
    GBps                  those bytes over lens_ms + emit_ms, beside the best plain 16-byte streaming read and write lines of
                          tools/probe/stream_probe.hip in the same run (stream_read_tbps, stream_write_tbps)
    encode_ms             wall time of the whole call: both kernels, the sizes down, the scan on the host, the offsets up
  Every result is decoded again on the device (SignalDecoder) and compared with the samples; the bytes themselves are the tests' business.
  --lib PATH measures another build of the library (make variant).
  --e2e runs the command on configs[1] (50 000 reads of 400 bases on average, k = 5) five ways and records wall time, the signal bytes
  copied from the device and the file's size: --sig_compress none and svb-zd, zlib on top of svb-zd at -t 1 and -t 16, zlib alone at -t 16.
  static: registers, scratch and LDS of the kernels (tools/isa_stats.py).
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_tbps():
    """(best plain 16-byte read, best plain 16-byte write) of the probe in TB/s, None where the probe cannot be built or run"""
    exe = os.path.join(ROOT, "tools", "probe", "stream_probe")
    if not os.path.exists(exe):
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", exe, exe + ".hip"], capture_output=True, text=True)
        if r.returncode:
            return None, None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    best = lambda tag: max([float(m.group(1)) for m in re.finditer(r"^%s plain.*?([0-9.]+) TB/s" % tag, r.stdout, re.M)], default=None)
    return best("A"), best("W")


def static_picture():
    src = os.path.join(ROOT, "poregen_amd", "csrc", "pg_svbenc.hip")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), src], capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired):
        return None
    return None if r.returncode else r.stdout.splitlines()


def bench(name, b, reps, rd, wr):
    import torch
    from poregen_amd.engine import SignalDecoder, SignalEncoder
    sig = torch.from_numpy(b.sig).cuda()
    soff = b.sig_off.astype(np.uint64)
    enc, dec = SignalEncoder(), SignalDecoder()
    lens = emit = wall = None
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blocks, boff = enc.encode(sig, soff)
        dt = time.perf_counter() - t0
        a, c = enc.kernel_ms()
        if i:
            lens = a if lens is None else min(lens, a); emit = c if emit is None else min(emit, c); wall = dt if wall is None else min(wall, dt)
    out, so, bad = dec.decode(blocks, boff)
    assert not bad.any() and np.array_equal(so, soff) and torch.equal(out, sig)
    n, nb = int(b.sig.size), int(blocks.numel())
    moved = 4 * n + nb
    res = dict(shape=name, reads=int(b.n_reads), samples=n, pieces=int(sum(max(1, -(-int(x) // 4096)) for x in np.diff(soff.astype(np.int64)))), block_bytes=nb,
               bytes_per_sample=round(nb / n, 4), lens_ms=lens, emit_ms=emit, encode_ms=wall * 1e3, bytes=moved, GBps=round(moved / ((lens + emit) * 1e-3) / 1e9, 1),
               lens_GBps=round(2 * n / (lens * 1e-3) / 1e9, 1), emit_GBps=round((2 * n + nb) / (emit * 1e-3) / 1e9, 1),
               lens_share_of_stream_read=round(2 * n / (lens * 1e-3) / (rd * 1e12), 3) if rd else None,
               emit_share_of_stream_write=round((2 * n + nb) / (emit * 1e-3) / (wr * 1e12), 3) if wr else None)
    enc.close(); dec.close()
    return res


def e2e(reads, read_len):
    """the command, five ways, on files of its own in a temporary directory"""
    exe = os.path.join(ROOT, "bin", "poregen")
    rng = np.random.default_rng(5)
    out = []
    with tempfile.TemporaryDirectory(prefix="sigenc_e2e") as d:
        kmers = [""]
        for _ in range(5):
            kmers = [p + c for p in kmers for c in "ACGT"]
        lv, sd = rng.integers(60000, 130000, 1024), rng.integers(1000, 3000, 1024)
        with open(os.path.join(d, "k5.model"), "w") as f:
            f.write("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{lv[i] / 1000:.3f}\t{sd[i] / 1000:.3f}\n" for i, km in enumerate(kmers)))
        with open(os.path.join(d, "ref.fa"), "w") as f:
            f.write(">chr\n" + "".join("ACGT"[i] for i in rng.integers(0, 4, 1 << 20)) + "\n")
        ways = (("none", []), ("svb-zd", ["--sig_compress", "svb-zd"]), ("zlib+svb-zd -t 1", ["--sig_compress", "svb-zd", "--compress", "zlib", "-t", "1"]),
                ("zlib+svb-zd -t 16", ["--sig_compress", "svb-zd", "--compress", "zlib", "-t", "16"]), ("zlib -t 16", ["--compress", "zlib", "-t", "16"]))
        for name, opts in ways:
            path = os.path.join(d, "out.blow5")
            t0 = time.perf_counter()
            r = subprocess.run([exe, "simulate", "-o", path, "-n", str(reads), "--read_len", str(read_len), "--seed", "3", *opts, os.path.join(d, "k5.model"), os.path.join(d, "ref.fa")],
                               capture_output=True, text=True, timeout=600)
            dt = time.perf_counter() - t0
            if r.returncode:
                raise SystemExit("simulate failed: " + r.stderr)
            m = re.search(r"samples=(\d+)", r.stderr)
            c = re.search(r"copied from the device=(\d+)", r.stderr)
            samples = int(m.group(1))
            out.append(dict(way=name, wall_s=round(dt, 3), samples=samples, signal_bytes_copied=int(c.group(1)) if c else 2 * samples, file_bytes=os.path.getsize(path)))
            os.remove(path)
            print("done:", name, out[-1]["wall_s"], "s", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-samples", type=int, default=0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--no-static", action="store_true", help="leave out the compile that tools/isa_stats.py needs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigenc_bench.json"))
    a = ap.parse_args()
    if a.lib:
        from poregen_amd import _abi
        _abi.LIB_PATH = os.path.abspath(a.lib)
    import torch
    from poregen_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("sigenc_bench: no GPU (this tool measures the device path; there is no CPU fallback)")
    rd, wr = stream_tbps()
    res = {"device_name": torch.cuda.get_device_name(0), "lib": a.lib, "stream_read_tbps": rd, "stream_write_tbps": wr, "static": None if a.lib or a.no_static else static_picture(), "runs": []}
    n1 = 50000 if not a.max_samples else max(1, a.max_samples // 4000)
    lens = synth.ragged_lengths(a.max_samples) if a.max_samples else synth.ragged_lengths()
    for name, make in (("configs[1]: %d x 4000 samples" % n1, lambda: synth.make_batch_fast(n1, 4000, seed=20251003)), ("ragged", lambda: synth.make_ragged_fast(lens))):
        res["runs"].append(bench(name, make(), a.reps, rd, wr))
        print("done:", name, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if a.e2e:
        res["e2e"] = e2e(n1, 400)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
