#!/usr/bin/env python3
"""mvops_bench.py -- the move-table expansion (pg_mvops_expand) and `poregen gmove --reform` on one MI355X.

  device   the batch already in HBM (CUDA tensors, PG_LOC_DEVICE): wall time of MoveExpander.expand -- its five kernels plus the
           read-back of the statuses -- as the best of --reps runs after one warm-up, at the configs[1] shape (50 000 reads x 800 table
           elements) and at a ragged shape (lognormal table lengths from 400 to 200 000 elements, the same total). Bytes per second over
           the bytes the kernels must move at least once (tables read twice, packed bases read, ops + op_t + seq written) beside the
           8 TB/s HBM peak DESIGN.md uses.
  cli      wall time, median of --runs, of `gmove --reform reads.bam` against the two-step route on the same files:
           `reform -c -k 1 --stride 0` plus `gmove --fastq reads.fastq reads.paf`, both commands' times added.
  ref      (--cases ref, or --ref) the projection onto the reference (pg_mvops_project) beside the expansion on the same device batches: the two
           shapes above with CIGARs drawn at 5 % edits, and the ragged shape with clean single-word CIGARs. Per call the HIP-event time
           on the expander's stream (the kernels, the small copies of offsets and statuses between them and the host's share in between)
           and the wall time, best of --reps after one warm-up. Bytes per second over 4 B read plus 5 B written per output op plus, per
           CIGAR word, its 4 B and its two 4-byte prefixes written once and read once; beside it the best plain streaming read of
           tools/probe/stream_probe.hip in the same run. One box, one run: a first look, not a bound -- no counters were read.
  strands  (--ref --strands) pg_mvops_project_stranded beside pg_mvops_project on the same device batch -- every read forward, and every
           second read reversed -- as HIP-event times on the expander's stream, best of --reps after one warm-up, every repeat kept (their
           spread is the noise floor of the box). With --lib PATH the library at PATH is loaded instead; one that lacks the stranded entry
           point (the parent commit's, `make variant`) is timed on pg_mvops_project alone: run the two alternating, tools/ab_lib.sh style.
           Then pg_refseq_slice: the slices of the same reads (ref_len from the projection, every second read reversed) cut from
           contigs in HBM, device arrays in, HIP-event and wall time per call and bytes of slice per second over them -- the KERNEL time
           is rocprofv3's, from a run of its own -- beside what today's host loop does for the same reads: per read a slice of the contig
           appended to one buffer (numpy on the host here; the product's is FastxIndex::fetch + vector::insert), then one upload and a
           synchronise, on the host clock.
Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def tables(lengths, seed=1, density=0.45):
    """Back-to-back tables of the given lengths, each opened by a move, with as many bases as moves and a signal that ends with the table."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    mv = (rng.random(int(off[-1])) < density).astype(np.int8)
    mv[off[:-1].astype(np.int64)] = 1
    moves = np.add.reduceat(mv.astype(np.int64), off[:-1].astype(np.int64))
    l_seq = moves.astype(np.uint32)
    nb = (l_seq.astype(np.int64) + 1) // 2
    boff = np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64)
    codes = np.array([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88], np.uint8)
    seqb = codes[rng.integers(0, 16, int(boff[-1]))]
    n = len(lengths)
    stride = np.full(n, 10, np.int32)
    ts = np.full(n, 100, np.uint64)
    ns = (np.asarray(lengths, np.uint64) - 1) * 10 + 100 + 7
    return dict(mv=mv, mv_off=off, stride=stride, ns=ns, ts=ts, l_seq=l_seq, flag=np.zeros(n, np.uint32), seq_bytes=seqb, byte_off=boff[:-1].copy())


def bench_device(name, lengths, reps):
    import torch
    from poregen_amd.engine import MoveExpander
    a = tables(lengths)
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    ex = MoveExpander()
    best = None
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ex.expand(t["mv"], t["mv_off"], t["stride"], t["ns"], t["ts"], t["l_seq"], t["flag"], t["seq_bytes"], t["byte_off"], rna=True)
        dt = time.perf_counter() - t0
        if i and (best is None or dt < best):
            best = dt
    assert r.n_refused == 0 and r.n_ops == int(a["l_seq"].sum())
    moved = 2 * a["mv"].size + a["seq_bytes"].size + r.n_ops * (4 + 1 + 1)
    ex.close()
    return dict(shape=name, reads=len(lengths), table_bytes=int(a["mv"].size), ops=int(r.n_ops), seconds=best, bytes_moved=int(moved),
                bytes_per_s=moved / best, share_of_hbm_peak=moved / best / HBM_PEAK)


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


def cigars(l_seq, rate, seed=5):
    """One CIGAR per read over its l_seq bases: M runs of geometric length with a 1..3-base I or D between them (rate = 0: one word LM)."""
    rng = np.random.default_rng(seed)
    words, off = [], [0]
    for L in l_seq.tolist():
        if rate <= 0 or L < 4:
            w = [L << 4]
        else:
            n_runs = max(1, int(L * rate))
            cuts = np.sort(rng.choice(np.arange(1, L), size=min(n_runs, L - 1), replace=False))
            runs = np.diff(np.concatenate([[0], cuts, [L]]))
            w, kinds, lens = [], rng.random(len(runs)), rng.integers(1, 4, len(runs))
            for i, m in enumerate(runs.tolist()):
                if i and kinds[i] < 0.5 and m > int(lens[i]):
                    w.append(int(lens[i]) << 4 | 1); m -= int(lens[i])
                elif i:
                    w.append(int(lens[i]) << 4 | 2)
                w.append(m << 4)
        words += w; off.append(len(words))
    return np.array(words, np.uint32), np.array(off, np.uint64), rng.integers(0, 1 << 24, len(l_seq)).astype(np.int32)


def bench_ref(name, lengths, rate, reps):
    import torch
    from poregen_amd.engine import MoveExpander
    a = tables(lengths)
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    cg, cg_off, pos = cigars(a["l_seq"], rate)
    d_cg, d_off, d_pos = torch.from_numpy(cg.view(np.int32)).cuda(), torch.from_numpy(cg_off.view(np.int64)).cuda(), torch.from_numpy(pos).cuda()
    ex = MoveExpander()
    stream = torch.cuda.Stream()
    ex.set_stream(stream)
    best = dict(expand_event_ms=None, expand_wall_ms=None, project_event_ms=None, project_wall_ms=None)

    def timed(key, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        wall, ev = (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
        return r, wall, ev

    for i in range(reps + 1):
        mo, w, e = timed("expand", lambda: ex.expand(t["mv"], t["mv_off"], t["stride"], t["ns"], t["ts"], t["l_seq"], t["flag"], t["seq_bytes"], t["byte_off"], rna=True))
        if i:
            best["expand_wall_ms"] = min(w, best["expand_wall_ms"] or w); best["expand_event_ms"] = min(e, best["expand_event_ms"] or e)
        pr, w, e = timed("project", lambda: ex.project(mo, d_cg, d_off, d_pos, rna=True))
        if i:
            best["project_wall_ms"] = min(w, best["project_wall_ms"] or w); best["project_event_ms"] = min(e, best["project_event_ms"] or e)
    assert mo.n_refused == 0 and pr.n_refused == 0 and int(pr.n_match_host.sum()) + int(((cg & 15) == 1).sum()) + int(((cg & 15) == 2).sum()) == pr.n_ops
    moved = pr.n_ops * (4 + 5) + cg.size * (4 + 2 * 4 * 2)
    out = dict(shape=name, cigars="clean: one word per read" if rate <= 0 else f"{rate:.0%} edits", reads=len(lengths), ops_in=int(mo.n_ops), ops_out=int(pr.n_ops),
               cigar_words=int(cg.size), bytes_moved=int(moved), **best)
    out["project_bytes_per_s"] = moved / (best["project_event_ms"] * 1e-3)
    out["project_share_of_hbm_peak"] = out["project_bytes_per_s"] / HBM_PEAK
    ex.close()
    return out


def _event_timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return r, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def bench_strands(name, lengths, rate, reps):
    import torch
    from poregen_amd.engine import MoveExpander
    a = tables(lengths)
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    cg, cg_off, pos = cigars(a["l_seq"], rate)
    n = len(lengths)
    d_cg, d_off, d_pos = torch.from_numpy(cg.view(np.int32)).cuda(), torch.from_numpy(cg_off.view(np.int64)).cuda(), torch.from_numpy(pos).cuda()
    fwd, half = torch.zeros(n, dtype=torch.uint8).cuda(), torch.from_numpy((np.arange(n) % 2).astype(np.uint8)).cuda()
    clen = torch.full((n,), 1 << 26, dtype=torch.int32).cuda()
    ex = MoveExpander()
    stream = torch.cuda.Stream()
    ex.set_stream(stream)
    mo = ex.expand(t["mv"], t["mv_off"], t["stride"], t["ns"], t["ts"], t["l_seq"], t["flag"], t["seq_bytes"], t["byte_off"], rna=False)
    calls = {"project": lambda: ex.project(mo, d_cg, d_off, d_pos)}
    if hasattr(ex._lib, "pg_mvops_project_stranded") and not getattr(ex._lib.pg_mvops_project_stranded, "missing", False):
        calls["stranded_all_forward"] = lambda: ex.project(mo, d_cg, d_off, d_pos, reverse=fwd, contig_len=clen)
        calls["stranded_half_reverse"] = lambda: ex.project(mo, d_cg, d_off, d_pos, reverse=half, contig_len=clen)
    ev = {k: [] for k in calls}
    for i in range(reps + 1):
        for k, fn in calls.items():                        # alternating: every call sees the same box
            pr, _, e = _event_timed(stream, fn)
            assert pr.n_refused == 0
            if i:
                ev[k].append(e)
    ref_len, n_ops = pr.ref_len_host.copy(), int(pr.n_ops)
    ex.close()
    out = dict(shape=name, cigars=f"{rate:.0%} edits", reads=n, ops_out=n_ops, cigar_words=int(cg.size))
    for k, v in ev.items():
        out[k + "_event_ms"] = dict(best=min(v), median=statistics.median(v), worst=max(v), all=[round(x, 4) for x in v])
    return out, pos, ref_len


def bench_refseq(pos, ref_len, reps, n_contigs=8, contig_bases=1 << 25):
    import torch
    from poregen_amd.engine import RefSeq
    rng = np.random.default_rng(9)
    n = len(pos)
    contigs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, contig_bases)] for _ in range(n_contigs)]
    contig = (np.arange(n) % n_contigs).astype(np.int32)
    reverse = (np.arange(n) % 2).astype(np.uint8)
    rs = RefSeq()
    stream = torch.cuda.Stream()
    rs.set_stream(stream)
    for c in contigs:
        rs.add(c.tobytes())
    d = [torch.from_numpy(x).cuda() for x in (contig, pos.astype(np.int32), ref_len.astype(np.uint32).view(np.int32), reverse)]
    ev, wall = [], []
    for i in range(reps + 1):
        r, w, e = _event_timed(stream, lambda: rs.slices(*d))
        if i:
            ev.append(e); wall.append(w)
    n_seq = r.n_seq
    # today's host loop for the same reads (all forward: it has no complement): slice, append, upload, synchronise
    host = []
    for i in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parts = [contigs[c][p:p + m] for c, p, m in zip(contig.tolist(), pos.tolist(), ref_len.tolist())]
        buf = np.concatenate(parts)
        off = np.concatenate([[0], np.cumsum(ref_len.astype(np.int64))])
        torch.from_numpy(buf).cuda(); torch.from_numpy(off).cuda()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    assert buf.size == n_seq
    rs.close()
    return dict(reads=n, slice_bytes=int(n_seq), contigs=n_contigs, contig_bases=contig_bases, half_reversed=True,
                slice_event_ms=dict(best=min(ev), median=statistics.median(ev), worst=max(ev)), slice_wall_ms=dict(best=min(wall), median=statistics.median(wall)),
                slice_bytes_per_s_over_event_time=n_seq / (min(ev) * 1e-3), host_loop_numpy_wall_ms=dict(best=min(host), all=[round(x, 3) for x in host]),
                hbm_peak_bytes_per_s=HBM_PEAK, note="event time holds three launches, the 8-byte read-back and two stream synchronises; the copy kernel's own time is rocprofv3's")


def bench_cli(n_reads, runs, tmp):
    from poregen_amd import synth
    b = synth.make_batch_fast(n_reads, kind="rna004", seed=11)
    b.target_start = np.zeros_like(b.target_start)
    pre = os.path.join(tmp, "mv")
    synth.write_bam(b, pre + ".bam", block_bytes=60000)
    synth.write_blow5(b, pre + ".blow5")
    with open(pre + ".fastq", "w") as f:
        for r in range(b.n_reads):
            s = synth.seq_string(b, r)
            f.write(f"@r{r}\n{s}\n+\n{'I' * len(s)}\n")
    exe = os.path.join(ROOT, "bin", "poregen")
    opts = ["--rna", "-k", "5", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "1000000", "--index_end", "1023"]   # a slice: every read is read

    def timed(cmd):
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return time.perf_counter() - t0

    one, two, parts = [], [], []
    for i in range(runs + 1):
        for d in ("o1", "o2"):
            shutil.rmtree(os.path.join(tmp, d), ignore_errors=True)
        a = timed([exe, "gmove", "--reform", pre + ".blow5", pre + ".bam"] + opts + [os.path.join(tmp, "o1")])
        r = timed([exe, "reform", "-c", "-k", "1", "--stride", "0", "--rna", "-o", pre + ".paf", pre + ".bam"])
        g = timed([exe, "gmove", "--fastq", pre + ".fastq", pre + ".blow5", pre + ".paf"] + opts + [os.path.join(tmp, "o2")])
        if i:
            one.append(a); two.append(r + g); parts.append((r, g))
    same = subprocess.run(["diff", "-rq", os.path.join(tmp, "o1"), os.path.join(tmp, "o2")], capture_output=True).returncode == 0
    return dict(reads=n_reads, samples=int(b.sig_off[-1]), runs=runs, one_step_median_s=statistics.median(one), two_step_median_s=statistics.median(two),
                reform_median_s=statistics.median(p[0] for p in parts), gmove_paf_median_s=statistics.median(p[1] for p in parts),
                one_step_s=one, two_step_s=two, outputs_equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cli-reads", type=int, default=20000)
    ap.add_argument("--cases", default="device,cli")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref", action="store_true", help="the projection onto the reference beside the expansion (= --cases ref)")
    ap.add_argument("--strands", action="store_true", help="with --ref: pg_mvops_project_stranded beside pg_mvops_project, and pg_refseq_slice (= --cases strands)")
    ap.add_argument("--lib", default=None, help="another libpgmove build to load (make variant); one without the stranded entry points is timed on pg_mvops_project alone")
    args = ap.parse_args()
    if args.ref:
        args.cases = "strands" if args.strands else "ref"
    if args.lib:
        import ctypes
        from poregen_amd import _abi

        class _Missing:                                      # a symbol the library at --lib does not have: bound, never called
            missing = True

        class _Older(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if name.startswith("pg_"):
                        return _Missing()
                    raise
        _abi.LIB_PATH = os.path.abspath(args.lib)
        _abi.C.CDLL = _Older
    out = {}
    if "strands" in args.cases.split(","):
        st, pos, ref_len = bench_strands("configs[1]: 50000 x 800", np.full(50000, 800, np.int64), 0.05, args.reps)
        out["strands"] = st
        out["lib"] = args.lib or "poregen_amd/libpgmove.so"
        if not args.lib:
            out["refseq"] = bench_refseq(pos, ref_len, args.reps)
    if "ref" in args.cases.split(","):
        rng = np.random.default_rng(3)
        ragged = np.clip(rng.lognormal(7.6, 1.0, 200000), 400, 200000).astype(np.int64)
        ragged = ragged[:int(np.searchsorted(np.cumsum(ragged), 50000 * 800)) + 1]
        out["ref"] = [bench_ref("configs[1]: 50000 x 800", np.full(50000, 800, np.int64), 0.05, args.reps), bench_ref("ragged 400..200000", ragged, 0.05, args.reps),
                      bench_ref("ragged 400..200000", ragged, 0.0, args.reps)]
        out["stream_read_tbps"] = stream_read_tbps()
    if "device" in args.cases.split(","):
        rng = np.random.default_rng(3)
        ragged = np.clip(rng.lognormal(7.6, 1.0, 200000), 400, 200000).astype(np.int64)
        ragged = ragged[:int(np.searchsorted(np.cumsum(ragged), 50000 * 800)) + 1]
        out["device"] = [bench_device("configs[1]: 50000 x 800", np.full(50000, 800, np.int64), args.reps), bench_device("ragged 400..200000", ragged, args.reps)]
    if "cli" in args.cases.split(","):
        tmp = tempfile.mkdtemp(prefix="mvops_bench", dir=args.tmp)
        try:
            out["cli"] = bench_cli(args.cli_reads, args.runs, tmp)
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
