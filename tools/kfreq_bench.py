#!/usr/bin/env python3
"""kfreq_bench.py -- throughput of `poregen kmer_freq` on one MI355X, in GB/s of FASTQ bytes.

A seeded synthetic FASTQ (lognormal read lengths, 0.1 % N, headers and qualities like the fixtures) of --gb gigabytes is made in
memory. Measured, each as the best of --reps runs after one warm-up:
  device      the bytes already in HBM (a torch.uint8 tensor, PG_LOC_DEVICE), k = 5, 9, 12, and a homopolymer file (one read of A)
              at k = 5 and 9; finish() (the D2H of the 4^k counts and the odd keys) is inside the time. Share of the 8 TB/s HBM peak
              next to the byte rate.
  host        the bytes in page-locked host memory (PG_LOC_HOST), k = 9, next to a plain copy of the same bytes to the device
              (torch copy_ from pinned memory = hipMemcpyAsync) measured in the same run: the H2D ceiling.
  cli         bin/poregen kmer_freq 9 FILE with --sort 0 and --sort 1, output to /dev/null, the file written to --tmp and read once
              before timing (page cache).
  cpu         one core: numpy rolling 2-bit codes + bincount over the sequence lines of the first --cpu-mb megabytes.
  reads       the same reads in the packed form of a BAM record (KmerCounter.submit_reads, two bases per byte): device-resident at
              k = 5, 9, 12 and from page-locked host memory at k = 9, each next to the FASTQ path on the same reads in the same run
              (rates in G bases/s, since the two forms differ in bytes per base), and the CLI on a BAM of the first --bam-mb
              megabytes of the FASTQ (written here with zlib level 1) next to the CLI on that FASTQ.
  fasta       a seeded synthetic FASTA (60-column lines, ~200-byte headers, lognormal record lengths, 0.1 % N) through
              KmerCounter.submit_fasta next to the FASTQ above through submit, in the same run: device-resident and from page-locked
              host memory, k = 5 and 9. Rates in G windows/s (the windows counted, from the result itself): a FASTA is nearly all
              sequence, a FASTQ about half, so bytes per second do not compare.
--cases picks a subset of device,host,cli,cpu,reads,fasta; the default is all but fasta, which has a profile of its own:
    tools/kfreq_bench.py --cases fasta --out profiles/kfreq_fasta_bench.json
Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(n_bytes, seed=1, n_rate=0.001):
    rng = np.random.default_rng(seed)
    parts, total, i = [], 0, 0
    lut = np.frombuffer(b"ACGT", np.uint8)
    while total < n_bytes:
        m = 4096
        lens = np.clip(rng.lognormal(8.5, 0.8, m), 50, 200_000).astype(np.int64)
        seq = lut[rng.integers(0, 4, int(lens.sum()))]
        seq[rng.random(seq.size) < n_rate] = ord("N")
        qual = rng.integers(35, 75, seq.size).astype(np.uint8)
        o = 0
        for L in lens:
            hdr = b"@%08x-1f2e-4d3c-9b8a-%012d runid=0f1e2d3c read=%d ch=%d start_time=2023-01-01T00:00:00Z\n" % (i, i, i, i % 512)
            rec = hdr + seq[o:o + L].tobytes() + b"\n+\n" + qual[o:o + L].tobytes() + b"\n"
            parts.append(rec)
            total += len(rec); o += L; i += 1
            if total >= n_bytes:
                break
    return b"".join(parts)


def synth_fasta(n_bytes, seed=2, n_rate=0.001, width=60):
    """Records like a transcriptome FASTA: a header of about 200 bytes, the sequence wrapped at `width` columns."""
    rng = np.random.default_rng(seed)
    parts, total, i = [], 0, 0
    lut = np.frombuffer(b"ACGT", np.uint8)
    while total < n_bytes:
        lens = np.clip(rng.lognormal(8.5, 0.8, 4096), 50, 200_000).astype(np.int64)
        seq = lut[rng.integers(0, 4, int(lens.sum()))]
        seq[rng.random(seq.size) < n_rate] = ord("N")
        o = 0
        for L in lens:
            hdr = (b">ENST%011d.%d cdna chromosome:GRCh38:%d:%d:%d:1 gene:ENSG%011d.%d gene_biotype:protein_coding transcript_biotype:protein_coding "
                   b"gene_symbol:SYN%d description:synthetic record %d of the benchmark [Source:kfreq_bench;Acc:%08d]\n") % (i, i % 9, i % 22 + 1, i * 7, i * 7 + L, i, i % 5, i, i, i)
            body = seq[o:o + L]
            full = (L // width) * width
            lines = np.empty((L // width, width + 1), np.uint8)
            lines[:, :width] = body[:full].reshape(-1, width); lines[:, width] = 10
            rec = hdr + lines.tobytes() + (body[full:].tobytes() + b"\n" if L > full else b"")
            parts.append(rec)
            total += len(rec); o += L; i += 1
            if total >= n_bytes:
                break
    return b"".join(parts)


def packed_reads(data):
    """The sequence lines of a FASTQ as pg_kfreq_submit_reads takes them: (seq_bytes, byte_off, l_seq, reverse = 0)."""
    buf = np.frombuffer(data, np.uint8)
    nl = np.flatnonzero(buf == 10)
    starts = np.concatenate(([0], nl[:-1] + 1))[1::4]
    lens = (nl[1::4] - starts).astype(np.int64)
    lut = np.full(256, 15, np.uint8)
    for code, letter in enumerate(b"=ACMGRSVTWYHKDBN"):
        lut[letter] = code
    padded = lens + (lens & 1)
    first = np.concatenate(([0], np.cumsum(padded)[:-1]))            # nibble index of each read's first base
    nib = np.full(int(padded.sum()), 15, np.uint8)
    src = np.repeat(starts - np.concatenate(([0], np.cumsum(lens)[:-1])), lens) + np.arange(int(lens.sum()))
    dst = np.repeat(first - np.concatenate(([0], np.cumsum(lens)[:-1])), lens) + np.arange(int(lens.sum()))
    nib[dst] = lut[buf[src]]
    seq = (nib[0::2] << 4 | nib[1::2]).astype(np.uint8)
    return seq, (first // 2).astype(np.uint64), lens.astype(np.uint32), np.zeros(lens.size, np.uint8)


def write_bam(path, seq, off, lens):
    """A BAM of the packed reads (flag 4, qualities 0xff, no tags), BGZF blocks of <= 64 000 bytes at zlib level 1."""
    import struct
    import zlib
    with open(path, "wb") as f:
        def block(b):
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            c = co.compress(b) + co.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(c) + 25) + c + struct.pack("<II", zlib.crc32(b), len(b)))
        pend = bytearray(b"BAM\1" + struct.pack("<ii", 0, 0))
        for i in range(lens.size):
            n = int(lens[i]); name = b"r%d\0" % i
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, 4, n, -1, -1, 0) + name + seq[int(off[i]):int(off[i]) + (n + 1) // 2].tobytes() + b"\xff" * n
            pend += struct.pack("<i", len(body)) + body
            while len(pend) >= 64000:
                block(bytes(pend[:64000])); del pend[:64000]
        if pend:
            block(bytes(pend))
        block(b"")


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def cpu_counter(data, k, limit):
    """Single-core neighbour: the same windows, counted with numpy (ACGT windows only, the odd ones are skipped)."""
    buf = np.frombuffer(data[:limit], np.uint8)
    t = time.perf_counter()
    nl = np.flatnonzero(buf == 10)
    starts = np.concatenate(([0], nl[:-1] + 1))
    lut = np.full(256, 255, np.uint8)
    for c, v in zip(b"ACGT", range(4)):
        lut[c] = v
    hist = np.zeros(4 ** k, np.int64)
    for li in range(1, len(nl), 4):
        line = buf[starts[li]:nl[li]]
        if line.size < k:
            continue
        b = lut[line].astype(np.int64)
        ok = b != 255
        code = np.zeros(line.size - k + 1, np.int64)
        good = np.ones(line.size - k + 1, bool)
        for j in range(k):
            code = code * 4 + (b[j:j + line.size - k + 1] & 3)
            good &= ok[j:j + line.size - k + 1]
        hist += np.bincount(code[good], minlength=4 ** k)
    dt = time.perf_counter() - t
    return int(nl[-1]) + 1 if len(nl) else len(buf), dt, int(hist.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-mb", type=int, default=256)
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--bam-mb", type=int, default=256)
    ap.add_argument("--cases", default="device,host,cli,cpu,reads")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfreq_bench.json"))
    a = ap.parse_args()
    cases = set(a.cases.split(","))
    import torch
    from poregen_amd.engine import KmerCounter
    if not torch.cuda.is_available():
        raise SystemExit("kfreq_bench: no GPU (this tool measures the device path; there is no CPU fallback)")

    t0 = time.perf_counter()
    data = synth(int(a.gb * 1e9))
    n = len(data)
    res = {"bytes": n, "gen_s": round(time.perf_counter() - t0, 1), "device_name": torch.cuda.get_device_name(0), "peak_hbm_GBps": 8000}
    gbps = lambda nb, s: round(nb / s / 1e9, 2)

    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    if "device" in cases:
        res["device"] = {}
        for k in (5, 9, 12):
            kc = KmerCounter(k)
            s = timed(lambda: (kc.submit(dev), kc.finish()), a.reps)
            kc.close()
            res["device"][f"k{k}"] = {"s": round(s, 4), "GBps": gbps(n, s), "of_hbm_peak": round(n / s / 8e12, 4)}
        homo = torch.full((n,), ord("A"), dtype=torch.uint8, device="cuda")
        homo[0] = ord("@"); homo[1] = 10; homo[n - 1] = 10
        for k in (5, 9):
            kc = KmerCounter(k)
            s = timed(lambda: (kc.submit(homo), kc.finish()), a.reps)
            kc.close()
            res["device"][f"homopolymer_k{k}"] = {"s": round(s, 4), "GBps": gbps(n, s), "of_hbm_peak": round(n / s / 8e12, 4)}
        del homo

    pinned = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory()
    pin_np = pinned.numpy()
    if "host" in cases:
        kc = KmerCounter(9)
        s_host = timed(lambda: (kc.submit(pin_np), kc.finish()), a.reps)
        kc.close()
        s_h2d = timed(lambda: dev.copy_(pinned, non_blocking=True), a.reps)
        res["host_pinned"] = {"k9_s": round(s_host, 4), "k9_GBps": gbps(n, s_host), "h2d_GBps": gbps(n, s_h2d),
                              "fraction_of_h2d": round(s_h2d / s_host, 3)}

    if "fasta" in cases:
        fa = synth_fasta(n)
        fa_dev = torch.frombuffer(bytearray(fa), dtype=torch.uint8).cuda()
        fa_pin = torch.frombuffer(bytearray(fa), dtype=torch.uint8).pin_memory().numpy()
        fr = {"fasta_bytes": len(fa), "fastq_bytes": n}
        for k in (5, 9):
            kc = KmerCounter(k)
            windows = {}
            for name, submit, d_in, h_in in (("fasta", kc.submit_fasta, fa_dev, fa_pin), ("fastq", kc.submit, dev, pin_np)):
                submit(d_in)
                r = kc.finish()
                windows[name] = int(r.counts.sum()) + int(r.odd_counts.sum())
                s_d = timed(lambda: (submit(d_in), kc.finish()), a.reps)
                s_h = timed(lambda: (submit(h_in), kc.finish()), a.reps)
                fr[f"{name}_k{k}"] = {"windows": windows[name], "device_s": round(s_d, 4), "device_Gwindows": round(windows[name] / s_d / 1e9, 2),
                                      "device_GBps": gbps(len(fa) if name == "fasta" else n, s_d), "host_pinned_s": round(s_h, 4),
                                      "host_pinned_Gwindows": round(windows[name] / s_h / 1e9, 2)}
            kc.close()
            fr[f"fasta_over_fastq_device_k{k}"] = round(fr[f"fasta_k{k}"]["device_Gwindows"] / fr[f"fastq_k{k}"]["device_Gwindows"], 3)
        res["fasta"] = fr
        del fa_dev, fa_pin

    exe = os.path.join(ROOT, "bin", "poregen")

    def cli(args, timeout=600):
        t = time.perf_counter()
        r = subprocess.run([exe, "kmer_freq"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
        if r.returncode:
            raise SystemExit(r.stderr.decode()[-2000:])
        return time.perf_counter() - t

    if "reads" in cases:
        # the same reads, packed: bases per second is the common unit (FASTQ: >= 2 bytes per base, packed: 0.5)
        seq, off, lens, rev = packed_reads(data)
        bases = int(lens.sum())
        gb = lambda s: round(bases / s / 1e9, 2)
        rd = {"bases": bases, "reads": int(lens.size), "packed_bytes": int(seq.size + 13 * lens.size), "fastq_bytes": n}
        d_arrs = tuple(torch.from_numpy(x).cuda() for x in (seq, off, lens, rev))
        for k in (5, 9, 12):
            kc = KmerCounter(k)
            s_r = timed(lambda: (kc.submit_reads(*d_arrs), kc.finish()), a.reps)
            s_f = timed(lambda: (kc.submit(dev), kc.finish()), a.reps)
            kc.close()
            rd[f"device_k{k}"] = {"reads_s": round(s_r, 4), "reads_Gbases": gb(s_r), "fastq_s": round(s_f, 4), "fastq_Gbases": gb(s_f)}
        kc = KmerCounter(9)
        s_r = timed(lambda: (kc.submit_reads(seq, off, lens, rev), kc.finish()), a.reps)
        s_f = timed(lambda: (kc.submit(pin_np), kc.finish()), a.reps)
        kc.close()
        rd["host_k9"] = {"reads_s": round(s_r, 4), "reads_Gbases": gb(s_r), "fastq_pinned_s": round(s_f, 4), "fastq_pinned_Gbases": gb(s_f)}
        del d_arrs
        # the CLI on a BAM of the first reads next to the CLI on their FASTQ
        cut = int(np.searchsorted(np.cumsum(lens.astype(np.int64) * 2 + 110), a.bam_mb << 20)) + 1
        sub = data[:int(np.flatnonzero(np.frombuffer(data, np.uint8) == 10)[4 * min(cut, lens.size) - 1]) + 1]
        s_seq, s_off, s_lens, _ = packed_reads(sub)
        bam, fq = os.path.join(a.tmp, "kfreq_bench.bam"), os.path.join(a.tmp, "kfreq_bench_sub.fastq")
        write_bam(bam, s_seq, s_off, s_lens)
        with open(fq, "wb") as f:
            f.write(sub)
        sb = int(s_lens.sum())
        t_b = min(cli(["9", bam]) for _ in range(max(1, a.reps - 1)))
        t_f = min(cli(["9", fq]) for _ in range(max(1, a.reps - 1)))
        rd["cli_k9"] = {"bases": sb, "bam_bytes": os.path.getsize(bam), "fastq_bytes": len(sub), "bam_s": round(t_b, 3), "bam_Gbases": round(sb / t_b / 1e9, 3),
                        "fastq_s": round(t_f, 3), "fastq_Gbases": round(sb / t_f / 1e9, 3)}
        os.unlink(bam); os.unlink(fq)
        res["reads"] = rd
    del pinned, pin_np, dev
    torch.cuda.empty_cache()

    if "cli" in cases:
        path = os.path.join(a.tmp, "kfreq_bench.fastq")
        with open(path, "wb") as f:
            f.write(data)
        with open(path, "rb") as f:
            while f.read(1 << 26):
                pass
        res["cli"] = {}
        for sort in (0, 1):
            best = min(cli(["--sort", str(sort), "9", path]) for _ in range(max(1, a.reps - 1)))
            res["cli"][f"k9_sort{sort}"] = {"s": round(best, 3), "GBps": gbps(n, best)}
        t12 = cli(["--sort", "1", "12", path], timeout=900)
        res["cli"]["k12_sort1"] = {"s": round(t12, 3), "GBps": gbps(n, t12), "lines": 4 ** 12}
        os.unlink(path)

    if "cpu" in cases:
        nb, s, windows = cpu_counter(data, 9, a.cpu_mb << 20)
        res["cpu_numpy_1core_k9"] = {"bytes": nb, "s": round(s, 3), "GBps": gbps(nb, s), "windows": windows}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
