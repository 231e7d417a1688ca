"""Pooled dump files without a GPU. tests/pool_ref.py against tests/dumptext_ref.py on the concatenated bytes (the identity the feature is
defined by); the moment combination the library compiles (csrc/pg_pool.h, through _pg_hosttest.so) against pool_ref's integers and sstdev
text; the name checks and argument refusals of `poregen model --pool` and `poregen offsets`, which end before a device is asked for."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import dumptext_ref as R
import pool_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
MAXU = 4 * 10**15 - 1


def text(units, ev=3):
    """a strict file of these values, in events of `ev`"""
    out = []
    for i, u in enumerate(units):
        out.append(R.fmt(u) + (b";" if (i + 1) % ev == 0 or i + 1 == len(units) else b","))
    return b"".join(out)


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_pool_combine.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_char_p, C.c_size_t]
    L.pgt_pool_combine.restype = C.c_int
    return L


def test_geometry():
    out = (C.c_uint32 * 4)()
    K.hosttest().pgt_pool_levels(out)
    tile, direct, threads, max_l = (int(x) for x in out)
    assert tile % (2 * threads) == 0 and 0 < direct <= threads and max_l == 16


# ---- the oracle is the per-file reference of the concatenation ---------------------------------------------------------------------------
def small_pools():
    rng = random.Random(5)
    vals = lambda n, c=10**10, w=10**9: [c + rng.randrange(-w, w) for _ in range(n)]
    yield [text(vals(5)), text(vals(4))]
    yield [b"", b"", text(vals(3)), b"", text(vals(6))]
    yield [text([7]), text([9])]
    yield [text([7])]
    yield [b"", b""]
    yield [text(vals(40, c=-10**12)), text(vals(41, c=-10**12 + 5 * 10**8)), text(vals(1, c=-10**12))]
    yield [text([0, 0, 0]), text([0, 0])]
    yield [text([5, -5]), b"-0.00000000;", text([0])]                     # a negative zero, both middles 0: refused
    yield [text([5, 6]), b"-0.00000000;", text([7])]                      # a negative zero away from the middle: fine
    yield [text(vals(3)), b"1.5;", text(vals(3))]                         # a member outside the grammar
    yield [text(vals(3)), text([0, 1 << 40])]                             # a member the reduction declines (spread)
    yield [text([MAXU, MAXU - 1, MAXU - (1 << 40) + 1])]


@pytest.mark.parametrize("keep_first", [False, True])
def test_oracle_equals_the_per_file_reference_of_the_concatenation(keep_first):
    n_ok = 0
    for members in small_pools():
        p = P.pool(members, keep_first)
        whole = b"".join(members)
        e = R.expect(whole, keep_first)
        if any(P.member_declined(m) for m in members):
            assert p.status == P.REFUSED and p.refused == [P.member_declined(m) for m in members].index(True)
            continue
        if e == R.HOST:                                                  # the concatenation is strict: only the "-0" rule is left
            assert p.status == P.REFUSED and R.classify(members[p.refused])[2]
            continue
        if e.n_values == 0:
            assert p.status == P.EMPTY
            continue
        assert p.status == P.OK and (p.n, p.mid_lo, p.mid_hi, p.origin, p.sum1, p.sum2) == tuple(e)[:6]
        n_ok += 1
    assert n_ok >= 6


# ---- the moment combination --------------------------------------------------------------------------------------------------------------
def member_moments(units):
    """what the per-file reduction leaves with the first value kept: (n, origin, s1, s2)"""
    if not units:
        return 0, 0, 0, 0
    d = [u - units[0] for u in units]
    return len(units), units[0], sum(d), sum(x * x for x in d)


def combine(h, moments, drop_first, second):
    n = np.array([m[0] for m in moments], np.uint64); origin = np.array([m[1] for m in moments], np.int64); s1 = np.array([m[2] for m in moments], np.int64)
    lo = np.array([m[3] & (2**64 - 1) for m in moments], np.uint64); hi = np.array([m[3] >> 64 for m in moments], np.uint64)
    out = np.zeros(8, np.int64); num = np.zeros(2, np.uint64); sd = C.create_string_buffer(64)
    st = h.pgt_pool_combine(len(moments), n.ctypes.data, origin.ctypes.data, s1.ctypes.data, lo.ctypes.data, hi.ctypes.data, int(drop_first), second,
                            out.ctypes.data, num.ctypes.data, sd, 64)
    s2 = (int(out[6]) % 2**64 << 64) + int(out[5]) % 2**64
    return st, int(out[1]), int(out[2]) % 2**64, int(out[3]), int(out[4]), s2, (int(num[1]) << 64) + int(num[0]), sd.value.decode()


def check_combine(h, members_units, keep_first):
    want = P.pool([text(u) if u else b"" for u in members_units], keep_first)
    flat = [u for m in members_units for u in m]
    st, why, n, origin, s1, s2, num, sd = combine(h, [member_moments(u) for u in members_units], not keep_first, flat[1] if len(flat) > 1 else 0)
    assert st == want.status
    if st == P.OK:
        assert (n, origin, s1, s2) == (want.n, want.origin, want.sum1, want.sum2)
        assert num == n * s2 - s1 * s1 and sd == P.sstdev_text(want.n, want.sum1, want.sum2)
    return want


@pytest.mark.parametrize("keep_first", [False, True])
def test_combination_equals_the_oracle(h, keep_first):
    rng = random.Random(11)
    near = lambda c, n, w=10**9: [c + rng.randrange(-w, w) for _ in range(n)]
    # members with far-apart origins: the whole range of the fixed-point view between them
    assert check_combine(h, [near(-MAXU + 10**9, 50), near(MAXU - 10**9, 70), near(0, 30)], keep_first).status == P.OK
    # the dropped value is the extreme
    assert check_combine(h, [[MAXU] + near(MAXU - 10**11, 9, 10**8), near(MAXU - 10**11, 20, 10**8)], keep_first).status == P.OK
    assert check_combine(h, [[-MAXU, -MAXU + (1 << 40) - 1], near(5, 20, 4)], keep_first).status == P.OK
    # empty members first, so that the dropped value and the origin come from later ones
    assert check_combine(h, [[], [], [123456789], [], near(10**10, 12)], keep_first).status == P.OK
    assert check_combine(h, [[], [5], [], [7, 9]], keep_first).status == P.OK
    # pools of one and of two values
    one = check_combine(h, [[], [42]], keep_first)
    assert one.status == (P.OK if keep_first else P.EMPTY)
    two = check_combine(h, [[42], [], [-58]], keep_first)
    assert two.status == P.OK and two.n == (2 if keep_first else 1)
    assert P.sstdev_text(two.n, two.sum1, two.sum2) == ("7.0710678118655e-07" if keep_first else "nan")
    assert check_combine(h, [[], []], keep_first).status == P.EMPTY
    for _ in range(40):
        mem = [near(rng.randrange(-MAXU + 10**10, MAXU - 10**10), rng.randrange(0, 9)) for _ in range(rng.randrange(1, 7))]
        check_combine(h, mem, keep_first)


def test_overflow_refusals(h):
    """synthetic per-file moments: no data of that size is needed"""
    WHY_COUNT, WHY_MOMENTS = 1, 2
    full = (1 << 23, 10**10, 0, 1 << 23)                                 # 2^23 values around 100: d = +-1
    # 512 such members hold 2^32 values: one too many with the first kept, 2^32 - 1 with it dropped
    st, why, *_ = combine(h, [full] * 512, False, 10**10)
    assert (st, why) == (P.REFUSED, WHY_COUNT)
    st, why, n, origin, s1, s2, num, sd = combine(h, [full] * 512, True, 10**10)
    assert st == P.OK and n == 2**32 - 1 and s2 == 2**32 and num == n * s2 and sd == P.sstdev_text(n, 0, s2)
    # n * sum d^2 - (sum d)^2 beyond 128 bits while every sum fits its field: one value at 0, 2^23 equal values at +far and at -far
    M = 1 << 23
    for far, fits in ((10**12, True), (39 * 10**14, False)):
        members = [(1, 0, 0, 0), (M, far, 0, 0), (M, -far, 0, 0)]
        s2 = 2 * M * far * far
        assert s2 < 2**128 and ((2 * M + 1) * s2 < 2**128) == fits
        st, why, n, origin, s1, got_s2, num, sd = combine(h, members, False, 0)
        want = P.from_sorted([0], 2 * M + 1, 0, 0, 0, 0, s2, [])
        if fits:
            assert st == P.OK == want.status and (n, origin, s1, got_s2, num) == (2 * M + 1, 0, 0, s2, (2 * M + 1) * s2) and sd == P.sstdev_text(n, 0, s2)
        else:
            assert (st, why) == (P.REFUSED, WHY_MOMENTS) and want.status == P.REFUSED
    # sum d beyond an int64: 2^23 values 3.9e15 units above the origin
    st, why, *_ = combine(h, [(M, 0, 0, 0), (M, 39 * 10**14, 0, 0)], False, 0)
    assert (st, why) == (P.REFUSED, WHY_MOMENTS)
    assert P.from_sorted([0], 2 * M, 0, 0, 0, M * 39 * 10**14, M * (39 * 10**14) ** 2, []).status == P.REFUSED


# ---- the commands' checks, made before a device is asked for -----------------------------------------------------------------------------
def make_dir(path, names):
    os.makedirs(path)
    for n in names:
        with open(os.path.join(path, n), "wb") as fh:
            fh.write(b"1.00000000,2.00000000;")
    return str(path)


def run(*args):
    r = subprocess.run([BIN] + list(args), capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


def test_cli_name_checks(tmp_path):
    good = make_dir(tmp_path / "good", ["ACGTA", "ACGTC"])
    lengths = make_dir(tmp_path / "lengths", ["AAAAA", "AAAC", "CCCCC"])
    letters = make_dir(tmp_path / "letters", ["AAAAA", "ACGNA", "CCCCC"])
    mixed = make_dir(tmp_path / "mixed", ["AAAAA", "AAATA", "AAAUA"])
    k17 = make_dir(tmp_path / "k17", ["A" * 17])
    for cmd in (["model", "--pool", "0:1"], ["offsets"]):
        for d, offender in ((lengths, "AAAC"), (letters, "ACGNA"), (mixed, "AAAUA")):
            rc, out, err = run(*cmd, d)
            assert rc == 1 and out == "" and offender + ":" in err and "HIP" not in err, (cmd, d, err)
    rc, out, err = run("offsets", k17)
    assert rc == 1 and out == "" and "17" in err
    for spec in ("5:1", "0:6", "3:3", "-1:2", "0:0", "2", "a:b", "1:2x"):
        rc, out, err = run("model", "--pool", spec, good)
        assert rc == 1 and out == "" and "--pool" in err, spec
    rc, out, err = run("model", "--pool", "0:1", "--dwell_model", str(tmp_path / "dw"), good)
    assert rc == 1 and out == "" and "--dwell_model" in err and not os.path.exists(tmp_path / "dw")
    # two directories whose union breaks the rule: the merged names are what is checked
    rc, out, err = run("offsets", good, make_dir(tmp_path / "rna", ["ACGUA"]))
    assert rc == 1 and "ACGUA:" in err


def test_reference_tables():
    files = {"AAC": text([10, 20, 30]), "AAG": text([40]), "CAG": text([100, 200]), "CCG": b""}
    assert P.pool_table(files, 0, 1, False) == "A\t3e-07\t1e-07\nC\t2e-06\tnan\n"
    assert P.pool_table(files, 2, 1, True, limit="5e-7") == "C\t2e-07\t1e-07\nG\t1e-06\t5e-7\n"
    assert P.pool_table(files, 2, 1, True, limit="1").endswith("G\t1e-06\t8.0829037686548e-07\n")
    t = P.offsets_table(files, False).split("\n")
    assert t[0] == "base\t0\tA\t2\t3\t3e-07\t1e-07" and t[2] == "base\t0\tG\t0\t0\t\t" and t[12:16] == ["spread\t0\t1.7e-06", "spread\t1\t", "spread\t2\t1.25e-06", "best\t0"]
    with pytest.raises(ValueError):
        P.check_names(["AAT", "AAU"])
    assert P.check_names(["AAU", "CCC"]) == (3, "ACGU")
