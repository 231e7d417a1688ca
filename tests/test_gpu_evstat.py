"""The event table on the GPU (pg_evstat.hip: k_ev_stats, k_ev_carry; pg_dmodel_finish_events; `poregen model --event_model`, `gmove
--event_model`) against tests/evstat_ref.py, exactly: every event's mean and standard deviation, every column of every file, every line of
the table; a refused file by its status and message, with the other files of its batch still right. Small synthetic dump text, placed on
the seams of the kernel's decomposition (the geometry comes from csrc/pg_evstat.h through the host test library)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import dumptext_ref as R
import evstat_ref as E
from poregen_amd import _abi, synth
from poregen_amd.engine import DumpModel, PgError, event_model_from_dumps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")


def geometry():
    out = (C.c_uint64 * 5)()
    K.hosttest().pgt_evstat_levels(out)
    return [int(x) for x in out]


MAX_LEN, MAX_DEV, LANE, TILE, BLOCK = geometry()
rng = random.Random(20261019)


def ev(n, centre=10**10, width=10**9):
    return [centre + rng.randrange(-width, width + 1) for _ in range(n)]


def ftext(events):
    return b"".join(b",".join(R.fmt(u) for u in e) + b";" for e in events)


def lens_file(lens, **kw):
    return ftext([ev(n, **kw) for n in lens])


@pytest.fixture(scope="module")
def dm():
    h = DumpModel(events=True, keep_events=True)
    yield h
    h.close()


def column_of(model, i):
    return (int(model.n_values[i]), int(model.mid_lo[i]), int(model.mid_hi[i]), int(model.origin[i]), int(model.sum1[i]),
            (int(model.sum2_hi[i]) << 64) + int(model.sum2_lo[i]))


def check(h, batches, keep_first=False):
    """lists of files (bytes), one list per submit, through one handle: every file against the reference. Returns the statuses."""
    for files in batches:
        off = np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)
        h.submit(b"".join(files), off)
    m, info = h.finish()
    t = h.finish_events()
    files = [f for b in batches for f in b]
    assert len(t.status) == len(files) == info.n_files and t.ev_mean.size == t.ev_sd.size == int(t.n_events.sum())
    at = 0
    for i, f in enumerate(files):
        want = E.table(f, keep_first)
        n = int(t.n_events[i])
        assert int(t.status[i]) == want.status, (i, f[:60], t.refusal[i])
        if want.status != E.ST_HOST:
            assert n == want.n_events, i
        if want.status:
            assert t.refusal[i].startswith("file %d:" % i) and all(p in t.refusal[i] for bit, p in E.PHRASE.items() if want.status & bit), t.refusal[i]
            assert not any(p in t.refusal[i] for bit, p in E.PHRASE.items() if not want.status & bit), t.refusal[i]
            assert column_of(t.means, i) == column_of(t.sds, i) == (0, 0, 0, 0, 0, 0)
            assert (t.means.median_text[i], t.means.sstdev_text[i], t.sds.median_text[i], t.sds.sstdev_text[i]) == ("", "", "", "")
        else:
            assert t.refusal[i] == ""
        if want.means:                                       # every event, also of a file whose columns the reduction declines
            assert t.ev_mean[at:at + n].tolist() == want.means and t.ev_sd[at:at + n].tolist() == want.sds, (i, f[:60])
        if not want.status:
            assert column_of(t.means, i) == tuple(want.mean_col) and column_of(t.sds, i) == tuple(want.sd_col), i
            got = "f\t%d\t%s\t%s\t%s\t%s\n" % (n, t.means.median_text[i], t.means.sstdev_text[i], t.sds.median_text[i], t.sds.sstdev_text[i])
            assert got == E.line("f", want), i
        at += n
    return [int(x) for x in t.status]


LENS = [2, 3, 63, 64, 65, 127, 128, 129, MAX_LEN]


def test_event_lengths_alone_and_mixed(dm):
    alone = [lens_file([n]) for n in LENS]
    assert check(dm, [alone]) == [0] * len(LENS)
    mixed = [lens_file(LENS), lens_file(LENS[::-1]), lens_file([129, 2, 128, 3, 127, 63, MAX_LEN, 65, 64, 2, 2, 2])]
    assert check(dm, [mixed]) == [0, 0, 0]
    assert check(dm, [[f] for f in mixed]) == [0, 0, 0]      # each in a batch of its own: other positions in the arena


@pytest.mark.parametrize("edge", [TILE, BLOCK, 3 * TILE, 2 * BLOCK])
def test_events_at_tile_and_workgroup_edges(dm, edge):
    """an event that ends one value before, exactly on and one value after the edge (so the next one begins before, on and after it),
    reached by one long event, by short ones, and with the file boundary on the edge"""
    files = []
    for delta in (-1, 0, 1):
        end = edge + delta
        files.append(lens_file([end, 9]))                                        # one event up to the edge (the file is first in its batch)
        files.append(lens_file([end - 40, 40, 2, TILE + 5]))                     # short events around it, one going on into the next tile
        files.append(lens_file([7] * ((end - 3) // 7) + [3 + (end - 3) % 7, 2]))
    batches = [[f] for f in files]
    # the file boundary itself on, before and behind the edge; and in the middle of a tile
    for delta in (-1, 0, 1):
        batches.append([lens_file([edge + delta - 20, 20]), lens_file([2]), lens_file([33, TILE, 2])])
    assert all(s == 0 for s in check(dm, batches))


def test_event_over_three_workgroups_and_the_longest_event(dm):
    files = [lens_file([BLOCK - 200, 2 * BLOCK + 100, 40]), lens_file([77, MAX_LEN, 5]), lens_file([MAX_LEN, MAX_LEN, 2, MAX_LEN]),
             lens_file([MAX_LEN, TILE - 1, MAX_LEN - 1])]
    assert check(dm, [files]) == [0, 0, 0, 0]
    assert check(dm, [[files[1]], [files[0]]]) == [0, 0]


def test_files_of_no_one_and_two_events(dm):
    files = [b"", lens_file([5]), lens_file([4, 9]), b"", b"", lens_file([2]), lens_file([2, 2]), b""]
    assert check(dm, [files]) == [0] * len(files)
    assert check(dm, [[b""], [b"", b""]]) == [0, 0, 0]                            # batches without a value
    # the table's text for them
    assert E.line("k", E.table(b"")) == "k\t0\t\t\t\t\n" and E.line("k", E.table(files[1])).count("nan") == 2


def test_many_files_over_several_submits(dm):
    files = []
    for i in range(300):
        n_ev = rng.choice([0, 1, 2, 3, 5, 8, 20])
        files.append(lens_file([rng.choice([2, 3, 5, 9, 17, 40, 70, 130]) for _ in range(n_ev)], centre=rng.randrange(-10**12, 10**12), width=rng.choice([1, 10**6, 10**9])))
    assert all(s == 0 for s in check(dm, [files[:100], files[100:101], files[101:250], files[250:]]))
    assert all(s == 0 for s in check(dm, [files]))


def test_values(dm):
    w = MAX_DEV
    files = [ftext([ev(9, centre=-10**12), ev(30, centre=-10**12 + 5, width=20)]), ftext([ev(30, centre=-5, width=20)] * 2),   # negative values
             ftext([ev(2, centre=-3 * 10**15, width=10**3), ev(77, centre=-3 * 10**15, width=10**10)]),
             ftext([[123456789] * 7, [-42] * 2, [0] * 130, [5] * MAX_LEN]),                                            # all equal: s = 0
             ftext([[7, 7 + w - 1]]), ftext([[-7 - (w - 1), -7]]),                                                      # the extreme-spread pair, alone in its file
             ftext([[3 * 10**15, 3 * 10**15 + 1]] * 3), ftext([[0, 1], [1, 0], [-1, 0], [0, 0, 0, 1], [0, 0, 0, 3]])]   # halves
    assert check(dm, [files]) == [0] * len(files)
    c = 3 << 38                                                                    # spreads 2^40 apart inside the sample model's window
    assert check(dm, [[ftext([[0, 0], [-c, c]]), files[0]]]) == [E.ST_DECLINED, 0]
    h = DumpModel(keep_first=True, events=True, keep_events=True)                  # the pair with its first value kept: the sample model declines the file
    try:
        assert check(h, [[files[4], files[0], files[1]]], keep_first=True) == [E.ST_HOST, 0, 0]
    finally:
        h.close()


def test_refusals_leave_the_other_files_right(dm):
    good = [lens_file([5, 70, 2]), lens_file([TILE + 3, 4]), lens_file([9] * 40)]
    one = ftext([ev(5), ev(1), ev(6)])
    many_ones = ftext([ev(1) for _ in range(3 * TILE)])                            # more event starts in a tile than a wave has lanes
    too_long = lens_file([3, MAX_LEN + 1, 3])
    far_too_long = lens_file([2 * MAX_LEN + 77])
    wide = ftext([[0, 5, MAX_DEV], [1, 2]])                                        # (2^41 from its event's first sample is 2^40 from the file's: the sample model declines it first)
    delimited = b"1.00000000,2.00000000:3.00000000,4.00000000;"                    # a -d file
    sci = b"1e2;"
    bad = [one, many_ones, too_long, far_too_long, wide, delimited, sci]
    want = [E.ST_ONE_SAMPLE, E.ST_ONE_SAMPLE, E.ST_TOO_LONG, E.ST_TOO_LONG, E.ST_HOST, E.ST_HOST, E.ST_HOST]
    files = []
    for i, b in enumerate(bad):
        files += [good[i % 3], b]
    files.append(good[0])
    st = check(dm, [files])
    assert st[1::2] == want and not any(st[0::2])
    assert check(dm, [[many_ones, good[1]], [too_long], [good[2], far_too_long, good[0]]]) == [E.ST_ONE_SAMPLE, 0, E.ST_TOO_LONG, 0, E.ST_TOO_LONG, 0]


def test_handle_without_the_flag():
    h = DumpModel()
    try:
        h.submit(b"1.00000000,2.00000000;", [0, 22])
        with pytest.raises(PgError) as e:
            h.finish_events()
        assert "PG_DMODEL_EVENTS" in str(e.value)
        m, info = h.finish()                                                       # and the handle goes on
        assert int(m.n_values[0]) == 1
    finally:
        h.close()


# ---- the commands ----------------------------------------------------------------------------------------------------------------------
def write_dir(path, files):
    os.makedirs(path)
    for name, data in files.items():
        with open(os.path.join(path, name), "wb") as fh:
            fh.write(data)
    return str(path)


def run(*args, env=None):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout, r.stderr


def test_cli_model_event_model(tmp_path):
    files = {"AAAAA": lens_file([5, 9, 30, 2]), "AAAAC": b"", "AAAAG": lens_file([12]), "AAAAT": lens_file([BLOCK + 7, 3, 3]),
             "AAACA": ftext([[100, 300], [200, 200, 200]]), "AAACC": lens_file([7] * 300, centre=-10**11)}
    d = write_dir(tmp_path / "d", files)
    want = E.event_table(files)
    assert isinstance(want, str) and "AAAAC\t0\t\t\t\t\n" in want and "AAACA\t2\t2e-06\t0\t7.05e-07\t9.9702056147303e-07\n" in want
    a, b, e = tmp_path / "a", tmp_path / "b", tmp_path / "e"
    assert run("model", d, "-o", a)[0] == 0
    rc, out, err = run("model", d, "-o", b, "--event_model", e)
    assert rc == 0, err
    assert e.read_text() == want and a.read_bytes() == b.read_bytes()
    # --keep_first changes the model, not the table; several batches change neither
    b2, e2 = tmp_path / "b2", tmp_path / "e2"
    assert run("model", d, "-o", b2, "--event_model", e2, "--keep_first", env=dict(os.environ, POREGEN_MODEL_BATCH="3000"))[0] == 0
    assert e2.read_text() == want and b2.read_bytes() != b.read_bytes()
    names, t, info = event_model_from_dumps([d], batch_bytes=2000)
    assert t.lines(names) == want and info.n_batches > 1


@pytest.mark.parametrize("name,data,phrase", [("one", ftext([[1, 2], [5]]), "one sample"), ("long", ftext([[3] * (MAX_LEN + 1)]), "longer than"),
                                               ("delim", b"1.00000000:2.00000000;", "on the host"), ("sci", b"1e2;", "on the host")],
                         ids=["one_sample", "too_long", "delimited", "scientific"])
def test_cli_refusal_writes_nothing(tmp_path, name, data, phrase):
    d = write_dir(tmp_path / "d", {"AAAAA": lens_file([5, 9]), "AAAAC": data, "AAAAG": lens_file([4])})
    o, e = tmp_path / "o", tmp_path / "e"
    rc, out, err = run("model", d, "-o", o, "--event_model", e)
    assert rc == 1 and out == "" and "AAAAC" in err and phrase in err, err
    assert not o.exists() and not e.exists()
    assert run("model", d, "-o", o)[0] == 0 and o.exists()                          # without the table the model is written as before


def test_gmove_event_model_equals_model_on_its_directory(tmp_path):
    """the synthetic k = 5 RNA set of test_gpu_dump_model.py"""
    b = synth.make_batch(300, kind="rna004", seed=31)
    pre = str(tmp_path / "in")
    synth.write_files(b, pre)
    out, ge, raw = tmp_path / "out", tmp_path / "ge", tmp_path / "raw"
    r = subprocess.run([BIN, "gmove", "-k", "5", "--rna", "--scaling", "1", "--sample_limit", "50", "--min_dur", "19", "--max_dur", "51", pre + ".slow5", pre + ".paf",
                        str(out), "--fastq", pre + ".fastq", "--file_limit", "1024", "--event_model", str(ge), "--raw_model", str(raw)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    me, mo = tmp_path / "me", tmp_path / "mo"
    rc, _, err = run("model", out / "dump", "-o", mo, "--event_model", me)
    assert rc == 0, err
    assert me.read_bytes() == ge.read_bytes() and mo.read_bytes() == raw.read_bytes()
    lines = me.read_text().splitlines()
    assert len(lines) == 1024 and sum(1 for l in lines if int(l.split("\t")[1]) >= 2) > 100
    files = {n: open(out / "dump" / n, "rb").read() for n in sorted(os.listdir(out / "dump"))[:64]}
    assert "".join(l + "\n" for l in lines[:64]) == E.event_table(files)
    rc, _, err = run("gmove", "--devices", "0,0", "--event_model", tmp_path / "x", pre + ".slow5", pre + ".paf", tmp_path / "out2")
    assert rc == 1 and "--event_model" in err and not (tmp_path / "out2").exists()


def test_engine_model_events_equals_the_reference_on_its_own_text(monkeypatch):
    """pg_model_events over a context's kept samples (doubles, converted as their "%.8f" text stands for them) against the reference on
    the dump text the same context prints"""
    monkeypatch.setenv("PGMOVE_HOLD_MIN_BYTES", "1")          # (as tests/test_gpu_text.py: a job this small keeps its samples on the device for pg_text)
    from poregen_amd.engine import GmoveEngine, GmoveParams, generate_kmers
    kmers = generate_kmers(5, rna=True)
    b = synth.make_batch(256, kind="rna004", seed=7)
    for parts in ([b], [b.slice_reads(0, 100), b.slice_reads(100, 101), b.slice_reads(101, 256)]):   # one batch; several, merged at finish
        eng = GmoveEngine(GmoveParams(kmers=kmers, kmer_size=5, rna=True, scaling=1, min_dur=20, max_dur=40, sample_limit=20))
        try:
            for part in parts:
                eng.submit(part)
            files = dict(zip(kmers, eng.text()))
            t = eng.model_events()
            assert not t.status.any() and int(t.n_events.sum()) > 1000
            assert t.lines(kmers) == E.event_table(files)
        finally:
            eng.close()
