"""`poregen subtool0` / `pa_stats` on the MI355X: the reference's own golden file, the CLI byte for byte against tests/pamean_ref.py on
every SLOW5 / BLOW5 flavour (duplicate ids, empty reads, digitisation 0, 10^6-sample reads, reads next to a %f rounding boundary), and
SignalMeans on host and device input: same means, the fallback count, a summary within 1e-13 of the exact one and independent of
batching."""
import os
import subprocess

import numpy as np
import pytest

import pamean_ref as R
from poregen_amd import synth
from poregen_amd.engine import SignalMeans, read_means

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
B5 = os.path.join(ROOT, "tests", "golden", "blow5")


def run(*args, cmd="subtool0", env=None):
    e = dict(os.environ, **(env or {}))
    return subprocess.run([BIN, cmd] + [str(a) for a in args], capture_output=True, env=e, timeout=600)


def records(seed=1, n=60, with_long=True):
    """ragged reads with real calibrations, duplicate ids, empty reads, digitisation-0 reads and (optionally) a 10^6-sample read"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.choice([0, 1, 2, 7, 100, 4000, 12_345, 70_000]))
        raw = rng.normal(600, 90, L).clip(-32768, 32767).astype(np.int16)
        dig, off, r = 2048.0, float(rng.integers(-260, -229)), float(rng.uniform(280, 285))
        out.append((f"read_{i % 45}", raw, dig, off, r))        # ids 0..14 appear twice
    out.append(("dig0_pos", np.array([500, 600], np.int16), 0.0, -243.0, 281.0))     # inf
    out.append(("dig0_mixed", np.array([500, -600, 3], np.int16), 0.0, 0.0, 281.0))  # inf - inf: -nan
    out.append(("range0", np.array([5, -7], np.int16), 2048.0, 0.0, 0.0))           # all zeros (one -0.0)
    out.append(("neg", rng.integers(-900, -100, 5000).astype(np.int16), 4096.0, 3.5, 1400.0))
    if with_long:
        out.append(("long", rng.normal(520, 70, 1_000_000).clip(-32768, 32767).astype(np.int16), 8192.0, 12.0, 1402.88))
    return out + R.boundary_reads(200_000, 2, seed=seed)


def batch(recs):
    sig = np.concatenate([r[1] for r in recs]).astype(np.int16)
    off = np.concatenate([[0], np.cumsum([len(r[1]) for r in recs])]).astype(np.uint64)
    return (sig, off, np.array([r[2] for r in recs]), np.array([r[3] for r in recs]), np.array([r[4] for r in recs]))


# ---- the CLI ----------------------------------------------------------------------------------------------------------------

def test_reference_golden_example():
    """test/example.exp is the reference's `poregen subtool0 test/example.blow5`: byte for byte. (Fails without the command.)"""
    r = run(os.path.join(B5, "example.blow5"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == open(os.path.join(B5, "example.exp"), "rb").read()


@pytest.mark.parametrize("kind", ["slow5", "none", "zlib+svb-zd", "zlib", "none+svb-zd", "zstd+svb-zd"])
def test_cli_matches_restatement(tmp_path, kind):
    recs = records(seed=3, with_long=kind in ("none", "zlib+svb-zd"))
    p = tmp_path / ("x.slow5" if kind == "slow5" else "x.blow5")
    if kind == "slow5":
        R.write_slow5(p, recs)
    else:
        rp, _, sp = kind.partition("+")
        if rp == "zstd" and synth.zstd_compress(b"x") is None:
            pytest.skip("no libzstd.so.1 on this machine")
        R.write_blow5(p, recs, rp, sp or "none")
    want = R.lines(recs)
    assert b"\t-nan\n" in want and b"\tinf\n" in want
    r = run(p)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == want
    if kind == "zlib+svb-zd":  # the options size nothing that changes the output; small device batches neither
        for args, env in ((["-K", 1], None), (["-K", 7], None), (["-B", "1K"], None), (["-t", 1], None), (["-t", 64, "-o", tmp_path / "o"], None),
                          (["--debug-break", 1, "-v", 0], None), ([], {"POREGEN_PAMEAN_BATCH_BYTES": "5000"})):
            r = run(*args, p, env=env)
            assert r.returncode == 0 and r.stdout == want, args


def test_adversarial_file_takes_the_loop(tmp_path):
    """reads whose exact mean and sequential mean print differently: the CLI prints the sequential text, and every one of them was
    finished by the loop"""
    recs = R.boundary_reads(200_000, 6, seed=29)
    assert len(recs) == 6
    for rid, raw, d, o, r in recs:
        assert R.fmt_f(R.exact_mean(raw, d, o, r)) != R.fmt_f(R.seq_mean(raw, d, o, r))
    p = tmp_path / "edge.blow5"
    R.write_blow5(p, recs)
    out = run(p)
    assert out.returncode == 0 and out.stdout == R.lines(recs)
    res = read_means(*batch(recs))
    assert res.n_fallback >= len(recs)
    assert [R.fmt_f(m) for m in res.means] == [R.fmt_f(R.seq_mean(*x[1:])) for x in recs]


def test_pa_stats_cli(tmp_path):
    recs = [x for x in records(seed=5) if x[2] != 0.0 and x[4] != 0.0]
    p = tmp_path / "x.blow5"
    R.write_blow5(p, recs, "zlib", "svb-zd")
    r = run(p, cmd="pa_stats")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    N, mean, sd = R.exact_summary(recs)
    got = r.stdout.decode().rstrip("\n").split("\t")
    assert len(got) == 2 and r.stdout == b"%.14g\t%.14g\n" % (float(got[0]), float(got[1]))
    assert abs(float(got[0]) - mean) <= 1e-13 * abs(mean) + 1e-12 and abs(float(got[1]) - sd) <= 1e-13 * sd + 1e-12
    for args in (["-K", 1], ["-B", "1K"]):
        assert run(*args, p, cmd="pa_stats").stdout == r.stdout
    assert run(p, cmd="pa_stats", env={"POREGEN_PAMEAN_BATCH_BYTES": "3000"}).stdout == r.stdout
    one = tmp_path / "one.blow5"
    R.write_blow5(one, [("a", np.array([5], np.int16), 2048.0, 0.0, 281.0), ("b", np.zeros(0, np.int16), 2048.0, 0.0, 281.0)])
    r = run(one, cmd="pa_stats")
    assert r.returncode == 1 and r.stdout == b""
    r = run(one)                                              # subtool0 has no such limit
    assert r.returncode == 0 and r.stdout == R.lines([("a", np.array([5], np.int16), 2048.0, 0.0, 281.0)])


def test_option_exit_codes(tmp_path):
    ex = os.path.join(B5, "example.blow5")
    gold = open(os.path.join(B5, "example.exp"), "rb").read()
    assert run("-V").stdout == b"subtool0 0.1.0\n"
    assert run("-h", ex).returncode == 0
    assert run().returncode == 1 and run(ex, ex).returncode == 1
    for bad in (["-K", 0], ["-t", -2], ["-B", 0]):
        assert run(*bad, ex).returncode == 1
    r = run("--no-such-option", ex)                           # getopt's message, then ignored
    assert r.returncode == 0 and r.stdout == gold and b"unrecognized option" in r.stderr
    assert run(tmp_path / "missing.blow5").returncode == 1
    exzd = tmp_path / "exzd.blow5"
    raw = bytearray(open(ex, "rb").read()); raw[14] = 2       # signal compression ex-zd: refused with a message
    exzd.write_bytes(bytes(raw))
    r = run(exzd)
    assert r.returncode == 1 and b"signal compression" in r.stderr


# ---- the library ------------------------------------------------------------------------------------------------------------

def test_device_input_and_batching_are_bit_identical():
    import torch
    recs = [x for x in records(seed=9) if x[2] != 0.0]
    sig, off, dig, offs, rng = batch(recs)
    host = read_means(sig, off, dig, offs, rng)
    dev = read_means(torch.from_numpy(sig).cuda(),
                     torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(dig).cuda(), torch.from_numpy(offs).cuda(),
                     torch.from_numpy(rng).cuda())
    empty = np.array([len(x[1]) == 0 for x in recs])
    assert np.isnan(host.means[empty]).all() and not np.isnan(host.means[~empty]).any()
    assert [R.fmt_f(m) for m, e in zip(host.means, empty) if not e] == [R.fmt_f(R.seq_mean(*x[1:])) for x in recs if len(x[1])]
    assert host.means.tobytes() == dev.means.tobytes() and host.n_fallback == dev.n_fallback
    assert (host.n_samples, host.mean, host.sstdev) == (dev.n_samples, dev.mean, dev.sstdev)
    # the same reads in batches of 1, 7 and 13 reads, one of them misaligned on the device: the same summary, bit for bit
    for step in (1, 7, 13):
        sm = SignalMeans()
        for a in range(0, len(recs), step):
            part = recs[a:a + step]
            b = batch(part)
            if step == 7 and a == 7:
                t = torch.from_numpy(np.concatenate([np.zeros(3, np.int16), b[0]])).cuda()[3:]
                sm.submit(t, torch.from_numpy(b[1].view(np.int64)).cuda(), *[torch.from_numpy(x).cuda() for x in b[2:]])
            else:
                sm.submit(*b)
        res = sm.finish()
        sm.close()
        assert res.means.tobytes() == host.means.tobytes()
        assert (res.n_samples, res.mean, res.sstdev) == (host.n_samples, host.mean, host.sstdev)
    N, mean, sd = R.exact_summary(recs)
    assert host.n_samples == N
    assert abs(host.mean - mean) <= 1e-13 * abs(mean) and abs(host.sstdev - sd) <= 1e-13 * sd


def test_summary_on_a_configs1_shaped_batch():
    b = synth.make_batch_fast(2000, 4000, seed=4)
    res = read_means(b.sig, b.sig_off, b.digitisation, b.offset, b.range)
    recs = [(str(i), b.sig[int(b.sig_off[i]):int(b.sig_off[i + 1])], b.digitisation[i], b.offset[i], b.range[i]) for i in range(b.n_reads)]
    N, mean, sd = R.exact_summary(recs)
    assert res.n_samples == N == b.n_samples
    assert abs(res.mean - mean) <= 1e-13 * abs(mean) and abs(res.sstdev - sd) <= 1e-13 * sd
    assert [R.fmt_f(m) for m in res.means] == [R.fmt_f(R.seq_mean(*x[1:])) for x in recs]
    assert res.n_fallback <= 0.01 * b.n_reads


def test_reuse_after_refusal():
    sm = SignalMeans()
    with pytest.raises(Exception):
        sm.submit(np.zeros(4, np.int16), np.array([0, 3, 1], np.uint64), np.ones(2), np.zeros(2), np.ones(2))   # decreasing offsets
    sm.submit(np.array([1, 2, 3], np.int16), np.array([0, 3], np.uint64), np.ones(1), np.zeros(1), np.ones(1))
    res = sm.finish()
    sm.close()
    assert R.fmt_f(res.means[0]) == b"2.000000" and res.n_samples == 3


def test_device_offsets_past_the_samples_are_refused():
    import torch
    sig = torch.zeros(10, dtype=torch.int16, device="cuda")
    off = torch.tensor([0, 4, 11], dtype=torch.int64, device="cuda")
    par = torch.ones(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        read_means(sig, off, par, par, par)
    with pytest.raises(ValueError):
        read_means(np.zeros(10, np.int16), np.array([0, 4, 11], np.uint64), np.ones(2), np.ones(2), np.ones(2))
