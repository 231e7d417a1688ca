"""`poregen subtool0` / `pa_stats` on any box: the decision that settles a read's mean text on the device (pg_pamean.h, through
_pg_hosttest.so) never settles a wrong text -- next to rounding boundaries, on ties, for negative means and for non-finite input --,
the host's sequential loop is the reference's, and the file-order walk visits every record, duplicates and empty reads included."""
import ctypes as C
import os

import numpy as np
import pytest

import pamean_cases as K
import pamean_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B5 = os.path.join(ROOT, "tests", "golden", "blow5")
BIN = os.path.join(ROOT, "bin", "poregen")


@pytest.fixture(scope="module")
def h():
    h = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    h.pgt_pa_shift.argtypes = [C.c_double]; h.pgt_pa_shift.restype = C.c_int
    h.pgt_pa_certify.argtypes = [C.c_uint64, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.POINTER(C.c_double)]
    h.pgt_pa_certify.restype = C.c_int
    h.pgt_pa_sequential_mean.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double]
    h.pgt_pa_sequential_mean.restype = C.c_double
    h.pgt_slow5_walk.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    h.pgt_slow5_walk.restype = C.c_long
    h.pgt_slow5_get.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]; h.pgt_slow5_get.restype = C.c_long
    return h


def certify(h, raw, dig, off, rng):
    """the device's decision for one read: None (falls back) or the mean it returns"""
    raw = np.asarray(raw, np.int16)
    c = h.pgt_pa_shift(off)
    s1 = int(raw.astype(np.int64).sum())
    sa = int(np.abs(raw.astype(np.int64) - c).sum())
    m = C.c_double()
    with np.errstate(all="ignore"):
        scale = float(np.float64(rng) / np.float64(dig))
    return m.value if h.pgt_pa_certify(raw.size, s1, sa, off, scale, C.byref(m)) else None


def check(h, raw, dig, off, rng):
    """a settled text is the reference's text; returns whether it was settled"""
    m = certify(h, raw, dig, off, rng)
    if m is not None:
        assert R.fmt_f(m) == R.fmt_f(R.seq_mean(raw, dig, off, rng)), (len(raw), dig, off, rng)
    return m is not None


def test_sequential_loop_is_the_reference(h):
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 4000, 100_000):
        raw = rng.integers(-2000, 3000, n).astype(np.int16)
        for dig, off, r in ((2048.0, -243.0, 281.345551), (8192.0, 13.7, 1402.882), (1.0, 0.0, 1.0), (0.0, 5.0, 281.0), (0.0, 0.0, 0.0)):
            got = h.pgt_pa_sequential_mean(raw.ctypes.data, n, dig, off, r)
            assert R.fmt_f(got) == R.fmt_f(R.seq_mean(raw, dig, off, r))
    # digitisation 0: inf, and 0 * inf / inf - inf give the x86 default NaN, which glibc prints as "-nan"
    raw = np.array([5, -5, 3], np.int16)
    assert R.fmt_f(h.pgt_pa_sequential_mean(raw.ctypes.data, 3, 0.0, 0.0, 281.0)) == b"-nan"
    raw = np.array([5, 6], np.int16)
    assert R.fmt_f(h.pgt_pa_sequential_mean(raw.ctypes.data, 2, 0.0, 0.0, 281.0)) == b"inf"
    # range 0 under negative samples: every x_i is -0.0, and the sum that starts at +0.0 stays +0.0
    raw = np.array([-5, -6, -32768], np.int16)
    assert R.fmt_f(h.pgt_pa_sequential_mean(raw.ctypes.data, 3, 2048.0, 0.0, 0.0)) == R.fmt_f(R.seq_mean(raw, 2048.0, 0.0, 0.0)) == b"0.000000"


def test_cells_just_inside_and_just_outside(h):
    """one sample, mean = value exactly: a value well inside a cell is settled with the right text; a value within the bound of the
    boundary is not settled; both sides of every boundary, positive and negative"""
    for j in (1, 7, 94_904_332, 123_456_789):
        for sign in (1.0, -1.0):
            for d in (0.4, 0.1, 1e-3, -1e-3, -0.1, -0.4):
                v = sign * (j + 0.5 + d) * 1e-6
                assert check(h, [1], 1.0, 0.0, v), v      # n = 1: the mean is scale itself; the bound is a few ulps
            v = sign * (j + 0.5) * 1e-6                    # (the double nearest the boundary: within ulps of it)
            check(h, [1], 1.0, 0.0, v)
    # wide reads: the bound grows with n (about n u mean = 4.4e-11 here); 1e-12 from a boundary is not settled, 1e-9 is
    raw = np.full(4000, 500, np.int16)
    for dd in (1e-9, -1e-9):
        off = (100.0000005 + dd) / (281.345551 / 2048.0) - 500.0
        assert certify(h, raw, 2048.0, off, 281.345551) is not None
        check(h, raw, 2048.0, off, 281.345551)
    for dd in (1e-12, -1e-12, 5e-12):
        off = (100.0000005 + dd) / (281.345551 / 2048.0) - 500.0
        assert certify(h, raw, 2048.0, off, 281.345551) is None
        check(h, raw, 2048.0, off, 281.345551)


def test_ties_are_never_settled(h):
    # 1/128 = 0.0078125 exactly: %f rounds the tie to even (0.007812); the cell test leaves it to the loop
    for v in (1 / 128, 3 / 128, -5 / 128, 12345 + 1 / 128):
        assert certify(h, [1], 1.0, 0.0, v) is None
        assert certify(h, [2, 0], 1.0, 0.0, v) is None


def test_zero_cell_sign(h):
    assert R.fmt_f(certify(h, [1], 1.0, 0.0, 1e-9)) == b"0.000000"
    assert R.fmt_f(certify(h, [1], 1.0, 0.0, -1e-9)) == b"-0.000000"
    assert certify(h, [0], 1.0, 0.0, 1.0) is None           # exactly zero: the sign is the loop's to decide
    assert certify(h, [5, -5], 1.0, 0.0, 1.0) is None
    assert certify(h, [3], 1.0, -3.0, 7.0) is None          # (3 - 3) * 7 = 0


def test_non_finite_input_is_never_settled(h):
    raw = [500, 510, 490]
    for dig, off, r in ((0.0, -243.0, 281.0), (2048.0, float("nan"), 281.0), (2048.0, float("inf"), 281.0),
                        (2048.0, -243.0, float("inf")), (2048.0, -243.0, float("nan")), (0.0, 0.0, 0.0)):
        assert certify(h, raw, dig, off, r) is None
    assert certify(h, raw, 2048.0, 1e300, 281.0) is None    # finite but far out: the bound says no
    assert certify(h, [], 2048.0, 0.0, 281.0) is None       # zero-length: never printed


def test_random_reads_never_get_a_wrong_text(h):
    """random lengths, calibrations and offsets, half of them tuned to sit next to a rounding boundary"""
    rng = np.random.default_rng(20261016)
    settled = 0
    for t in range(600):
        n = int(rng.integers(1, 3000))
        raw = rng.normal(rng.uniform(-800, 900), rng.uniform(1, 300), n).clip(-32768, 32767).astype(np.int16)
        dig = float(rng.choice([2048.0, 8192.0, 1.0, 4096.0]))
        r = float(rng.uniform(0.5, 2000.0)) * (1 if rng.random() < 0.9 else -1)
        off = float(rng.uniform(-500, 500))
        if t % 2:
            scale = r / dig
            target = (np.rint(R.exact_mean(raw, dig, off, r) * 1e6) + 0.5) * 1e-6 + float(rng.uniform(-1e-9, 1e-9))
            off = target / scale - float(raw.astype(np.float64).mean())
        settled += check(h, raw, dig, off, r)
    assert settled > 250    # the fast path is not vacuous


def test_boundary_reads_fall_back(h):
    for rid, raw, d, o, r in R.boundary_reads(200_000, 3):
        assert certify(h, raw, d, o, r) is None
        assert R.fmt_f(R.exact_mean(raw, d, o, r)) != R.fmt_f(R.seq_mean(raw, d, o, r))


def test_shift_rounds_to_nearest_and_clamps(h):
    """c is the integer nearest -offset (ties to even), clamped to +-2^20; a NaN gives a valid c as well"""
    for off, c in ((0.0, 0), (-0.0, 0), (-243.0, 243), (243.4, -243), (2.5, -2), (-3.5, 4), (1048575.5, -1048576), (-1048575.5, 1048576),
                   (1048576.5, -1048576), (-1048576.5, 1048576), (2e6, -1048576), (-2e6, 1048576), (1e300, -1048576), (-1e300, 1048576),
                   (float("inf"), -1048576), (float("-inf"), 1048576)):
        assert h.pgt_pa_shift(off) == c, off
    assert abs(h.pgt_pa_shift(float("nan"))) <= 1048576


def test_grid_holds_every_edge():
    """the shapes the GPU suite runs: every head / tail length, one trip of the vector loop +- 1 vector +- 1 sample, the piece +- 1"""
    assert set(range(25)) <= set(K.N_GRID) and {63, 64, 65, 8191, 8192, 8193, 12_293, 16_384, 16_385, 24_577, 70_001} <= set(K.N_GRID)
    assert {8 * v + e for v in (511, 512, 513) for e in (-1, 0, 1)} <= set(K.N_GRID)
    assert K.K_PIECE == 8192 and K.A_GRID == tuple(range(9)) and K.N_HUGE == 2 ** 20 + 1
    for family in K.FAMILIES:
        recs = K.grid_batch(family)
        assert len(recs[0][1]) == 0 and len(recs[-1][1]) == 0
        cur = 0
        seen = set()
        for rid, raw, *_ in recs:
            assert not (raw == 0).any()
            if rid.startswith("read_"):
                a, n = (int(v) for v in rid.split("_")[1:])
                assert cur % 8 == a % 8 and len(raw) == n
                seen.add((a, n))
            cur += len(raw)
        assert seen == {(a, n) for a in K.A_GRID for n in K.N_GRID}
        for a, n, (pad, read) in K.grid_cycles(family):
            assert len(pad[1]) == a and len(read[1]) == n
    low, alt, cap = (K.grid_cycles(f)[-1][2][1][1] for f in ("low", "alternating", "capped"))
    assert (low == -32768).all() and set(alt[::2]) == {-32768} and set(alt[1::2]) == {32767} and (cap[0], cap[-1]) == (32767, -32768)


def test_every_probe_shape_yields_both_probes(h):
    """the generator of the threshold probes (pamean_cases.py): every shape of the probe set gives a just-settled and a just-refused
    probe within its 20 draws, with the one-third margins on sa, and a settled probe's text is the reference's"""
    sh = K.shim()
    n_probes = 0
    for a, n in K.probe_shapes():
        for offset in K.PROBE_OFFSETS:
            for fi, family in enumerate(K.PROBE_FAMILIES):
                raw, rr, tries = K.probe_pair(sh, n, offset, family, np.random.default_rng([7, a, n, int(-offset), fi]))
                assert tries <= K.PROBE_TRIES and raw.size == n
                c = sh.shift(offset)
                _, s1, sa = sh.sums(raw, offset)
                dist = np.abs(raw.astype(np.int64) - c)
                d = int(dist.min())
                assert d >= 100 and not (raw == 0).any() and c == int(-offset)
                m = d // 3
                cert = lambda s, r: sh.certify(n, s1, s, offset, r) is not None      # noqa: E731
                # just settled: settled with room for the margin, refused once any one sample is counted twice
                r = rr["settled"]
                assert cert(sa + m, r) and cert(sa, r) and not cert(sa + d - m, r) and not cert(sa + d, r)
                assert check(h, raw, 1.0, offset, r)
                # just refused: refused with room for the margin, settled once any one sample is dropped
                r = rr["refused"]
                assert not cert(sa - m, r) and not cert(sa, r) and cert(sa - d + m, r) and cert(sa - d, r)
                assert not check(h, raw, 1.0, offset, r)
                n_probes += 2
    assert n_probes == 2 * 2 * 2 * (3 * 13 + 1)


def test_probe_batches_are_decided_as_built():
    """each probe sits at its a behind its pad read, and the host's decision is the one the batch is named after, pads included"""
    sh = K.shim()
    for kind, by_a in K.probe_batches().items():
        for a, recs in by_a.items():
            cur = 0
            for rid, raw, dig, off, rng in recs:
                if rid.startswith("probe_"):
                    assert cur % 8 == a
                if len(raw):
                    assert sh.settles(raw, dig, off, rng) == (kind == "settled"), (kind, a, rid)
                cur += len(raw)
            assert sh.n_fallback(recs) == (0 if kind == "settled" else sum(1 for r in recs if len(r[1])))


def walk(h, path):
    ids = C.create_string_buffer(1 << 20); lens = np.zeros(4096, np.uint64); err = C.create_string_buffer(512)
    n = h.pgt_slow5_walk(str(path).encode(), ids, len(ids), lens.ctypes.data, lens.size, err, len(err))
    assert n >= 0, err.value
    return ids.value.decode().split("\n")[:-1], lens[:n].tolist()


RECS = [("a", np.array([1, 2, 3], np.int16), 2048.0, -3.0, 281.0), ("empty", np.zeros(0, np.int16), 2048.0, 0.0, 281.0),
        ("a", np.array([-7], np.int16), 1.0, 0.5, 2.0), ("b", np.arange(1000, dtype=np.int16), 4096.0, 10.0, 1400.0),
        ("a", np.zeros(0, np.int16), 2048.0, 0.0, 281.0)]


@pytest.mark.parametrize("kind", ["slow5", "none", "zlib", "svb-zd", "zlib+svb-zd"])
def test_file_order_walk_keeps_duplicates_and_empty_reads(h, tmp_path, kind):
    p = tmp_path / ("x.slow5" if kind == "slow5" else "x.blow5")
    if kind == "slow5":
        R.write_slow5(p, RECS)
    else:
        rp = "zlib" if kind.startswith("zlib") else "none"
        sp = "svb-zd" if kind.endswith("svb-zd") else "none"
        R.write_blow5(p, RECS, rp, sp)
    ids, lens = walk(h, p)
    assert ids == [r[0] for r in RECS] and lens == [len(r[1]) for r in RECS]
    # the indexed reader (gmove's) still refuses the duplicate ids
    dor = np.zeros(3); raw = np.zeros(10, np.int16)
    assert h.pgt_slow5_get(str(p).encode(), b"b", dor.ctypes.data, raw.ctypes.data, 10) == -1


def test_reference_golden_through_the_walk_and_the_restatement(h):
    """test/example.blow5 walked in file order and restated == test/example.exp, the reference's own subtool0 output"""
    path = os.path.join(B5, "example.blow5")
    ids, lens = walk(h, path)
    recs = []
    for rid, n in zip(ids, lens):
        dor = np.zeros(3); raw = np.zeros(n, np.int16)
        assert h.pgt_slow5_get(path.encode(), rid.encode(), dor.ctypes.data, raw.ctypes.data, n) == n
        recs.append((rid, raw, *dor.tolist()))
    assert R.lines(recs) == open(os.path.join(B5, "example.exp"), "rb").read()


def s0(*args, cmd="subtool0"):
    import subprocess
    return subprocess.run([BIN, cmd] + [str(a) for a in args], capture_output=True)


@pytest.mark.parametrize("cmd", ["subtool0", "pa_stats"])
def test_options_that_never_reach_the_device(cmd):
    r = s0("-V", cmd=cmd)
    assert r.returncode == 0 and r.stdout == f"{cmd} 0.1.0\n".encode()
    r = s0("-h", cmd=cmd)
    assert r.returncode == 0 and f"Usage: poregen {cmd} reads.blow5".encode() in r.stdout
    for args in ([], ["a.blow5", "b.blow5"]):
        r = s0(*args, cmd=cmd)
        assert r.returncode == 1 and f"Usage: poregen {cmd}".encode() in r.stderr and r.stdout == b""
    for args in (["-K", "0"], ["-t", "0"], ["-B", "0"], ["-B", "-3K"], ["-K", "-1"]):
        r = s0(*args, os.path.join(B5, "example.blow5"), cmd=cmd)
        assert r.returncode == 1 and r.stdout == b"", args
    r = s0("/nonexistent/x.blow5", cmd=cmd)
    assert r.returncode == 1 and r.stdout == b""
