"""Pooled dump files on the GPU (pg_pool.hip): engine.DumpPool, `poregen model --pool` and `poregen offsets` against tests/pool_ref.py
(Python integers; tied to the per-file reference and to the library's moment combination by tests/test_pool_host.py). Every field of every
group is compared exactly; the commands are held to `poregen model` on the members' bytes concatenated."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import dumptext_ref as R
import pool_ref as P
from poregen_amd import _abi
from poregen_amd.engine import DumpPool, PgError, offsets_from_dumps, pool_from_dumps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
G = os.path.join(ROOT, "tests", "golden", "single_read")
NO = _abi.PG_POOL_NO_GROUP
MAXU = 4 * 10**15 - 1


def levels():
    out = (C.c_uint32 * 4)()
    K.hosttest().pgt_pool_levels(out)
    return int(out[0]), int(out[1])


T, DIRECT = levels()


def text(units, ev=4):
    units = list(units)
    return b"".join(R.fmt(u) + (b";" if (i + 1) % ev == 0 or i + 1 == len(units) else b",") for i, u in enumerate(units))


def rand_units(n, seed, center=9 * 10**9, width=2 * 10**9):
    rng = random.Random(seed)
    return [center + rng.randrange(-width, width) for _ in range(n)]


def check(files, gids, n_groups, keep_first, cuts=(), max_values=0):
    """files[i] in groups gids[i][l]; submitted in batches cut at the indices `cuts`. Every group of every labeling against the reference."""
    pool = DumpPool(n_groups, keep_first=keep_first, max_values=max_values)
    try:
        edges = [0] + list(cuts) + [len(files)]
        for a, b in zip(edges, edges[1:]):
            data, off, _ = K.batch(files[a:b])
            pool.submit(data, off, np.array(gids[a:b], np.uint32).reshape(b - a, len(n_groups)).T)
        res = pool.finish()
    finally:
        pool.close()
    compare(res, files, gids, n_groups, keep_first)
    return res


def compare(res, files, gids, n_groups, keep_first):
    m = res.model
    assert res.n_files_total == len(files) and res.n_bytes == sum(len(f) for f in files) and len(res.status) == sum(n_groups)
    assert res.n_values == sum(R.parsed_values(f) for f in files)
    base = 0
    for l, ng in enumerate(n_groups):
        for g in range(ng):
            mem = [i for i in range(len(files)) if gids[i][l] == g]
            want = P.pool([files[i] for i in mem], keep_first)
            s = base + g
            where = (l, g, mem[:8])
            assert int(res.status[s]) == want.status and int(res.n_files[s]) == len(mem), where
            assert int(res.refused_file[s]) == (mem[want.refused] if want.status == P.REFUSED else -1), where
            assert bool(res.refusal[s]) == (want.status == P.REFUSED), where
            got = (int(m.n_values[s]), int(m.mid_lo[s]), int(m.mid_hi[s]), int(m.origin[s]), int(m.sum1[s]), (int(m.sum2_hi[s]) << 64) + int(m.sum2_lo[s]))
            assert got == tuple(want)[2:], where
            assert (m.median_text[s], m.sstdev_text[s]) == P.texts(want), where
            assert int(m.dwell_n[s]) == 0 and np.isnan(m.dwell_median[s])
            if want.status == P.OK:
                assert abs(m.median[s] - float(m.median_text[s])) <= 1e-13 * abs(m.median[s])
        base += ng


def edge_files():
    """members of 0, 1, 2, DIRECT, DIRECT + 1, T - 1, T, T + 1 and 2T + 1 values, small ones between the large so that tiles hold several files"""
    sizes = [0, 1, 2, T - 1, 0, DIRECT, T, 1, DIRECT + 1, T + 1, 2, 3, 2 * T + 1, 0, 5, 1, T - 1, 2, DIRECT, 7]
    return [text(rand_units(n, 100 + i)) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("keep_first", [False, True], ids=["tail", "keep_first"])
def test_edges_one_labeling(keep_first):
    files = edge_files()
    gids = [[i % 4] for i in range(len(files))]
    gids[6] = [NO]                                        # a file in no group
    res = check(files, gids, [4], keep_first)
    assert list(res.status) == [P.OK] * 4
    check(files, gids, [4], keep_first, cuts=(3, 4, 11))  # the same over four submits: groups spread over them


@pytest.mark.parametrize("keep_first", [False, True], ids=["tail", "keep_first"])
def test_edges_nine_labelings(keep_first):
    files = edge_files()
    n_groups = [4, 1, 2, 3, 4, 5, 6, 7, 20]
    rng = random.Random(3)
    gids = [[i % 4, 0, i % 2] + [rng.randrange(ng) if rng.random() < 0.8 else NO for ng in n_groups[3:]] for i in range(len(files))]
    res = check(files, gids, n_groups, keep_first, cuts=(7, 13))
    assert P.EMPTY in list(res.status) and list(res.status).count(P.OK) >= 25


def scenarios():
    """pools as lists of members' units, each to be a group of its own"""
    one = 10**8
    return {
        "part_first_digit_2": [[5, -1, 1]],                                        # dropped 5: the middles are -1 and +1, keys apart in the top digit
        "part_first_digit_many": [[7] + [-1] * 40, [1] * 40],
        "part_last_digit": [[3 * one, 1000, 1001], [1000] * 9, [1001] * 9],
        "part_middle_digit": [[0, 65536 * 3, 65536 * 3 + 70000] * 5 + [0]],
        "all_equal_odd": [[42 * one] * 7, [42 * one] * (T + 1)],
        "all_equal_even": [[42 * one] * 6],
        "dropped_is_the_only_median": [[50, 10, 20], [80, 90]],                   # kept: 50 is the median; dropped: 20 and 80
        "dropped_from_the_third": [[], [], [11 * one], [12 * one, 13 * one]],
        "one_value": [[], [77]],
        "extremes": [[MAXU, MAXU - 5], [-MAXU, -MAXU + 5], [0]],
        "extremes_even": [[-MAXU], [MAXU], [MAXU - 1], [-MAXU + 1], [3]],
        "odd": [rand_units(2 * T + 1, 1), rand_units(DIRECT + 2, 2)],
        "even": [rand_units(2 * T + 1, 3), rand_units(DIRECT + 3, 4)],
        "negatives": [rand_units(300, 5, center=-10**10), rand_units(301, 6, center=10**10)],
        "empty": [[], []],
    }


@pytest.mark.parametrize("keep_first", [False, True], ids=["tail", "keep_first"])
def test_scenarios(keep_first):
    """every pool a group; the members dealt out round-robin, so that a group's files lie apart in the arena, over three submits"""
    sc = scenarios()
    names = list(sc)
    queues = [[(g, text(u) if u else b"") for u in sc[n]] for g, n in enumerate(names)]
    files, gids = [], []
    while any(queues):
        for q in queues:
            if q:
                g, f = q.pop(0)
                files.append(f); gids.append([g, g % 3])
    res = check(files, gids, [len(names), 3], keep_first, cuts=(len(files) // 3, 2 * len(files) // 3))
    by = {n: g for g, n in enumerate(names)}
    m = res.model
    mids = lambda n: (int(m.mid_lo[by[n]]), int(m.mid_hi[by[n]]))
    if keep_first:
        assert mids("dropped_is_the_only_median") == (50, 50) and mids("part_first_digit_2") == (1, 1)
    else:
        assert mids("dropped_is_the_only_median") == (20, 80) and mids("part_first_digit_2") == (-1, 1) and mids("part_first_digit_many") == (-1, 1)
        assert mids("part_last_digit") == (1000, 1001) and int(res.status[by["one_value"]]) == P.EMPTY
        assert mids("extremes_even") == (3, MAXU - 1)
    assert int(res.status[by["empty"]]) == P.EMPTY


@pytest.mark.parametrize("keep_first", [False, True], ids=["tail", "keep_first"])
def test_past_the_per_file_limit(keep_first):
    """one member of 2^18 values 33 times into one group: 2^23 + 2^18 values, more than one file may hold"""
    block = rand_units(1 << 18, 9, width=10**9)
    data = text(block, ev=32)
    off = [0, len(data)]
    pool = DumpPool([1, 2], keep_first=keep_first)
    try:
        for i in range(33):
            pool.submit(data, off, [[0], [i % 2]])
        res = pool.finish()
    finally:
        pool.close()
    assert res.n_values == 33 << 18 > R.MAX_VALUES
    want = P.pool_repeated(block, 33, keep_first)
    m = res.model
    assert want.status == P.OK == int(res.status[0]) and int(res.n_files[0]) == 33
    got = (int(m.n_values[0]), int(m.mid_lo[0]), int(m.mid_hi[0]), int(m.origin[0]), int(m.sum1[0]), (int(m.sum2_hi[0]) << 64) + int(m.sum2_lo[0]))
    assert got == tuple(want)[2:]
    assert (m.median_text[0], m.sstdev_text[0]) == P.texts(want)
    # the second labeling: the 17 even and the 16 odd submissions
    for g, reps in ((1, 17), (2, 16)):
        w = P.pool_repeated(block, reps, keep_first)                    # (every pool drops the first value of its own concatenation)
        assert (int(m.n_values[g]), int(m.mid_lo[g]), int(m.mid_hi[g]), int(m.sum1[g])) == (w.n, w.mid_lo, w.mid_hi, w.sum1)


def test_refusals():
    good = lambda seed: text(rand_units(50, seed))
    delimited = text(rand_units(6, 1))[:-1] + b":" + text(rand_units(3, 2))                # the -d form
    files = [good(1), good(2), delimited, good(3), text([5, -5]), b"-0.00000000;", text([0]), good(4), good(5), text([0, 1 << 40])]
    gids = [[0, 0], [1, 0], [1, 1], [1, 1], [2, 2], [2, 2], [2, 2], [3, 3], [0, 3], [4, 4]]
    for keep_first in (False, True):
        res = check(files, gids, [5, 5], keep_first, cuts=(4,))
        assert list(res.status[:5]) == [P.OK, P.REFUSED, P.REFUSED, P.OK, P.REFUSED] and list(res.refused_file[:5]) == [-1, 2, 5, -1, 9]
        assert "grammar" in res.refusal[1] and "negative zero" in res.refusal[2] and "2^40" in res.refusal[4] and "file 2" in res.refusal[1]
        assert list(res.status[5:]) == [P.OK, P.REFUSED, P.REFUSED, P.OK, P.REFUSED]


def test_arena_cap():
    first = [text(rand_units(900, 1)), text(rand_units(800, 2))]
    second = [text(rand_units(1500, 3))]
    third = [text(rand_units(300, 4))]
    gids = lambda n: np.zeros((1, n), np.uint32)
    for keep_first in (False, True):
        pool = DumpPool([1], keep_first=keep_first, max_values=2500)
        try:
            data, off, _ = K.batch(first)
            pool.submit(data, off, gids(2))
            data, off, _ = K.batch(second)
            with pytest.raises(PgError) as ei:
                pool.submit(data, off, gids(1))                               # 1700 + 1500 values pass the cap: nothing of it counts
            assert ei.value.status == _abi.PG_ERR_UNSUPPORTED and "max_values" in ei.value.text
            data, off, _ = K.batch(third)
            pool.submit(data, off, gids(1))                                   # the handle goes on
            res = pool.finish()
            compare(res, first + third, [[0]] * 3, [1], keep_first)
            assert res.n_values == 2000
            data, off, _ = K.batch(second)                                    # after finish the arena is empty again
            pool.submit(data, off, gids(1))
            compare(pool.finish(), second, [[0]], [1], keep_first)
        finally:
            pool.close()


def test_bad_arguments():
    lib = _abi.load()
    h = C.c_void_p()
    ng = np.array([2], np.uint32)
    assert lib.pg_pool_create(0, 17, C.c_void_p(ng.ctypes.data), 0, 0, C.byref(h)) == _abi.PG_ERR_INVALID_ARG
    assert lib.pg_pool_create(0, 1, C.c_void_p(ng.ctypes.data), 0, 2, C.byref(h)) == _abi.PG_ERR_INVALID_ARG
    pool = DumpPool([2])
    with pytest.raises(PgError) as ei:
        pool.submit(b"1.00000000;", [0, 11], [[2]])
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "group" in ei.value.text
    pool.submit(b"1.00000000,2.00000000;", [0, 22], [[1]])
    res = pool.finish()
    assert list(res.status) == [P.EMPTY, P.OK] and int(res.model.mid_lo[1]) == 2 * 10**8
    pool.close()


# ---- the commands ------------------------------------------------------------------------------------------------------------------------
def run(args, env=None):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout, r.stderr


def read_dirs(dirs):
    files = {}
    for d in dirs:
        for n in sorted(os.listdir(d)):
            files[n] = files.get(n, b"") + open(os.path.join(d, n), "rb").read()
    return files


def concatenated_dir(path, files, start, length):
    """one file per group: the members' bytes back to back in name order"""
    os.makedirs(path)
    for n in sorted(files, key=lambda x: x.encode()):
        with open(os.path.join(path, n[start:start + length]), "ab") as fh:
            fh.write(files[n])
    return path


@pytest.fixture(scope="module")
def dna5(tmp_path_factory):
    out = tmp_path_factory.mktemp("pool_dna") / "out"
    rc, _, err = run(["gmove", "-k", "5", "--file_limit", "1024", "--sample_limit", "5000", f"{G}/reads.slow5", f"{G}/guppy_move.paf", "--fastq", f"{G}/read_0.fastq", out])
    assert rc == 0, err
    return str(out / "dump")


@pytest.fixture(scope="module")
def rna5(tmp_path_factory):
    from test_gpu_dump_model import gmove_rna5
    tmp = tmp_path_factory.mktemp("pool_rna")
    return [str(gmove_rna5(tmp, name, seed)[0] / "dump") for name, seed in (("a", 31), ("b", 32))]


_serial = itertools.count()


def identity(tmp_path, dirs, start, length, extra=(), env=None):
    files = read_dirs(dirs)
    assert sum(1 for f in files.values() if f) >= 20
    cat = concatenated_dir(tmp_path / ("cat%d" % next(_serial)), files, start, length)
    rc, got, err = run(["model", "--pool", "%d:%d" % (start, length)] + list(extra) + list(dirs), env=env)
    assert rc == 0, err
    rc, want, err = run(["model"] + list(extra) + [cat])
    assert rc == 0 and "n_host_files: 0" in err, err
    assert got == want and got.count("\n") == len({n[start:start + length] for n in files})
    assert got == P.pool_table(files, start, length, bool(extra))
    return got


def test_cli_pool_equals_model_on_the_concatenation(tmp_path, dna5, rna5):
    a = identity(tmp_path, [dna5], 1, 3)
    assert identity(tmp_path, [dna5], 1, 3, extra=["--keep_first"]) != a
    assert "T" in a and "U" not in a
    small = dict(os.environ, POREGEN_MODEL_BATCH="20000")                     # many batches: groups spread over the submits
    assert identity(tmp_path / "b", [dna5], 1, 3, env=small) == a
    identity(tmp_path, [dna5], 0, 5)                                          # every file a group of its own
    u = identity(tmp_path, rna5[:1], 1, 3)                                    # an ACGU directory
    assert "U" in u and "T" not in u
    assert identity(tmp_path / "two", rna5, 1, 3) != u                        # two directories: a name's files back to back
    lines, res = pool_from_dumps(rna5, 1, 3)
    assert lines == identity(tmp_path / "py", rna5, 1, 3) and res.n_files_total == len(read_dirs(rna5))


def test_cli_offsets(tmp_path, dna5, rna5):
    for dirs, extra in (([dna5], []), ([dna5], ["--keep_first"]), (rna5, [])):
        rc, got, err = run(["offsets"] + extra + dirs)
        assert rc == 0, err
        assert got == P.offsets_table(read_dirs(dirs), bool(extra))
        assert got.count("\n") == 4 * 5 + 5 + 1 and "n_pooled_values" in err
        assert offsets_from_dumps(dirs, keep_first=bool(extra))[0] == got
    out = tmp_path / "o.tsv"
    rc, got2, err = run(["offsets", "-o", out, "-t", "3"] + rna5)
    assert rc == 0 and got2 == "" and out.read_text() == got


def test_cli_refused_group(tmp_path):
    d = tmp_path / "d"
    os.makedirs(d)
    for n, data in (("AAC", text([1, 2, 3])), ("AAG", b"1.00000000:2.00000000;"), ("CAG", text([4, 5]))):
        (d / n).write_bytes(data)
    out = tmp_path / "out.tsv"
    rc, got, err = run(["model", "--pool", "0:1", "-o", out, d])
    assert rc == 1 and got == "" and not out.exists() and "group A" in err and "AAG" in err
    rc, got, err = run(["offsets", d])
    assert rc == 1 and got == "" and "AAG" in err
    with pytest.raises(PgError):
        pool_from_dumps([d], 0, 1)
    assert P.pool_table(read_dirs([d]), 0, 1, False) == (P.REFUSED, "A", "AAG")
