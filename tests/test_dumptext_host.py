"""The dump-text parser of `poregen model` without a GPU. The field rule the kernels compile (csrc/pg_dumptext.h, through _pg_hosttest.so)
against tests/dumptext_ref.py on mutated files; dumptext_ref.py against oracle/model_oracle.c on the files of tests/dumptext_cases.py;
and the placement claims of those cases, so that the GPU suite (tests/test_gpu_dumptext_edges.py) stands on checked ground."""
import ctypes as C
import os
import random
import subprocess
from decimal import Decimal, getcontext
from fractions import Fraction

import pytest

import dumptext_cases as K
import dumptext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(os.environ.get("PG_ORACLE_DIR") or os.path.join(ROOT, "oracle"), "model_oracle")
SEPS = (ord(","), ord(";"))


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_model_texts.argtypes = [C.POINTER(C.c_longlong), C.c_size_t, C.c_char_p, C.c_char_p, C.c_size_t]
    L.pgt_dump_model_host.argtypes = [C.POINTER(C.c_char_p), C.c_size_t, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.pgt_dump_model_host.restype = C.c_long
    return L


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    if not os.path.exists(ORACLE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])


def test_geometry():
    lane, tile, wg, min_field = K.levels()
    assert wg % tile == 0 and tile == 64 * lane and min_field == 11


# ---- the field rule ----------------------------------------------------------------------------------------------------------------------
def header_file(h, prefix, data):
    """the file `data` behind `prefix` by the header's rule, one call per separator: None, or (units, has_negzero)"""
    buf = prefix + data
    lo = len(prefix)
    u, nz = C.c_int64(), C.c_int()
    units, negzero, ok = [], False, True
    for i in range(lo, len(buf)):
        if buf[i] in SEPS:
            if h.pgt_dumptext_field(buf, i, lo, C.byref(u), C.byref(nz)):
                units.append(u.value); negzero |= bool(nz.value)
            else:
                ok = False
    if not ok or (data and data[-1] != ord(";")):
        return None
    return units, negzero


def same_as_ref(h, prefix, data):
    got, want = header_file(h, prefix, data), R.classify(data)
    assert (got is None) == (want is None), (prefix, data, got, want)
    if want is not None:
        assert got == (want[0], want[2]), (prefix, data, got, want)
    return want is not None


ALPHABET = b"0123456789.,;-+e :\n"
PREFIXES = (b"12345", b"1.5", b"-", b"3.0000000", b"")


def seed_file(rng):
    out = []
    for _ in range(rng.randrange(0, 5)):
        kind = rng.randrange(6)
        ip = (rng.randrange(10), rng.randrange(40_000_000), rng.randrange(39_999_990, 40_000_010), rng.randrange(10**8), 0, rng.randrange(1000))[kind]
        text = b"%s%0*d.%08d" % (b"-" if rng.random() < 0.3 else b"", rng.choice((1, 1, 2, 8)), ip, rng.choice((0, 0, 1, 99999999, rng.randrange(10**8))))
        out.append(text + (b";" if rng.random() < 0.4 else b","))
    if out and rng.random() < 0.9:
        out[-1] = out[-1][:-1] + b";"
    return b"".join(out)


def mutate(data, rng):
    b = bytearray(data)
    for _ in range(rng.choice((0, 1, 1, 1, 2, 3))):
        op, c = rng.randrange(3), rng.choice(ALPHABET)
        if op == 0 and b:
            b[rng.randrange(len(b))] = c
        elif op == 1 and b:
            del b[rng.randrange(len(b))]
        else:
            b.insert(rng.randrange(len(b) + 1), c)
    return bytes(b)


def test_field_rule_against_the_reference_on_mutated_files(h):
    """200 000 files: strict by the header (every separator's field parses, the last byte is ';') iff strict by the reference's regular
    expression, and then the same units and the same negative-zero flag; the bytes in front of the file belong to no file"""
    rng = random.Random(20261019)
    n, strict = 200_000, 0
    for i in range(n):
        strict += same_as_ref(h, PREFIXES[i % len(PREFIXES)], mutate(seed_file(rng), rng))
    assert n // 10 < strict < n * 9 // 10, strict         # both outcomes are exercised


def test_every_length_of_the_integer_part(h):
    for nd in range(0, 11):
        for sign in (b"", b"-"):
            for digits in (b"1" * nd, b"0" * nd, b"3" + b"9" * (nd - 1) if nd else b"", b"4" + b"0" * (nd - 1) if nd else b"", b"0" + b"9" * (nd - 1) if nd else b""):
                field = sign + digits + b".00000001"
                for prefix in PREFIXES:
                    strict = [same_as_ref(h, prefix, f) for f in (field + b";", b"1.00000000," + field + b";", field + b"," + field + b";2.00000000;")]
                    want = 1 <= nd <= 8 and int(digits) < 40_000_000
                    assert strict == [want] * 3, (field, prefix)


# ---- the reference against the oracle ----------------------------------------------------------------------------------------------------
def model_texts(h, units):
    med = C.create_string_buffer(64); sd = C.create_string_buffer(64)
    h.pgt_model_texts((C.c_longlong * len(units))(*units), len(units), med, sd, 64)
    return med.value.decode(), sd.value.decode()


def exact_sstdev(units):
    getcontext().prec = 80
    n = len(units)
    s1 = sum(units); s2 = sum(u * u for u in units)
    var = Fraction(n * s2 - s1 * s1, n * (n - 1)) / 10**16
    return (Decimal(var.numerator) / Decimal(var.denominator)).sqrt()


def sstdev_agrees(mine, oracle, units):
    """compare_raw_model's rule (tests/test_gpu_model.py): equal texts, or one unit of the 14th digit apart with the exact text the correctly
    rounded exact value"""
    if mine == oracle:
        return True
    if mine in ("", "nan") or oracle in ("", "nan"):
        return False
    x, y = Decimal(mine), Decimal(oracle)
    if abs(x - y) > Decimal(1).scaleb(max(x.adjusted(), y.adjusted()) - 13):
        return False
    exact = exact_sstdev(units)
    return abs(x - exact) <= Decimal(1).scaleb(exact.adjusted() - 13) / 2


def write_dir(path, files):
    os.makedirs(path)
    names = ["f%06d" % i for i in range(len(files))]
    for name, data in zip(names, files):
        with open(os.path.join(path, name), "wb") as f:
            f.write(data)
    return names


def oracle_columns(d, mode, *args):
    out = subprocess.run([ORACLE, mode, str(d)] + list(args), capture_output=True, check=True).stdout.decode()
    return [l.split("\t")[1:] for l in out.split("\n")[:-1]]


@pytest.mark.parametrize("name", ["D", "E", "F", "G"])
def test_reference_against_the_oracle(tmp_path, h, name):
    """Every file of the family (each distinct file once), written to a directory: where the reference says device, the exact median and
    stddev of its integers print the oracle's texts and its events give the oracle's dwell line. The oracle drops the first value, so this
    is keep_first = False. The host path (pg_dumphost.h), which finishes the other files, prints the oracle's lines for all of them."""
    files = list(dict.fromkeys(f for b in K.family(name) for f in b[2]))
    d = tmp_path / name
    write_dir(str(d), files)
    stats, dw = oracle_columns(d, "stats", "1e9"), oracle_columns(d, "dwell")
    assert len(stats) == len(files) == len(dw)
    n_dev = 0
    for data, (o_med, o_sd), (o_dwell,) in zip(files, stats, dw):
        e = R.expect(data, False)
        if e == R.HOST:
            continue
        n_dev += 1
        units = R.classify(data)[0][1:]
        assert e.n_values == len(units)
        assert o_dwell == ("" if e.dwell_n == 0 else "%.14g" % e.dwell_median), data[:60]
        if not units:
            assert (o_med, o_sd) == ("", ""), data[:60]
            continue
        med, sd = model_texts(h, units)
        if max(abs(u) for u in units) >= 10**15:
            # values of 1e7 and beyond: strtold is up to 3.6e-12 off each of them and the oracle's texts with it, so only
            # the integers are compared: the reference's against a parse by decimal arithmetic, the median's text against theirs
            assert units == [int(Decimal(x.decode()).scaleb(8)) for x in data.replace(b";", b",").split(b",")[1:-1]]
            exact = (Decimal(e.mid_lo + e.mid_hi) / 2).scaleb(-8)
            assert abs(Decimal(med) - exact) <= Decimal(1).scaleb(exact.adjusted() - 13) / 2, (med, exact)
            continue
        assert med == o_med, (data[:60], med, o_med)
        assert sstdev_agrees(sd, o_sd, units), (data[:60], sd, o_sd)
    assert n_dev > len(files) // 4
    arr = (C.c_char_p * 1)(os.fsencode(str(d)))
    out = C.create_string_buffer(1 << 22); err = C.create_string_buffer(1024)
    assert h.pgt_dump_model_host(arr, 1, 0, b"1e9", 0, 2, out, len(out), err, len(err)) >= 0, err.value
    assert [l.split("\t")[1:] for l in out.value.decode().split("\n")[:-1]] == stats


def test_pairs_of_family_d_come_to_what_the_issue_states():
    for first, second, want in K.D_PAIRS:
        assert R.classify(first) is None
        assert (R.classify(second) or [None])[0] == want


# ---- the cases are where they claim to be ------------------------------------------------------------------------------------------------
def test_every_family_has_cases():
    for name in K.FAMILIES:
        fam = K.family(name)
        assert len(fam) > 0
        for data, off, files in fam:
            assert off[0] == 0 and off[-1] == len(data) and len(off) == len(files) + 1 and b"".join(files) == data
            K.representative(name)
    assert len(K.family("A")) == 3 * 21 * 2 * 2 and len(K.family("B")) == 3 * 35 * 3 and len(K.family("D")) == 4 * 17


def test_pad():
    for L in list(range(1, 11)) + [20, 21]:
        with pytest.raises(AssertionError):
            K.pad(L)
    for L in [0] + list(range(11, 20)) + list(range(22, 300)) + [K.TILE, K.WG - 1, K.WG + 1]:
        f = K.pad(L)
        assert len(f) == L and R.expect(f, True) != R.HOST and R.expect(f, False) != R.HOST
    assert R.expect(K.TAIL, False) != R.HOST and len(K.TAIL) > 2 * K.TILE


def test_family_a_puts_the_separator_on_the_stated_byte():
    seen = set()
    for (data, off, files), sep in K.family_a():
        assert data[sep] in SEPS
        field = K.F19 if data[sep - len(K.F19):sep] == K.F19 else K.F11
        assert data[sep - len(field):sep] == field and data[sep - len(field) - 1] in SEPS
        assert R.expect(files[-2], False) != R.HOST and R.expect(files[-2], True) != R.HOST       # the probe's file stays on the device
        begin = sep - len(field)
        assert off[-3] < begin and sep < off[-2]
        seen.add((sep, field, sep + 1 == off[-2]))
    assert seen == {(E + d, f, last) for E in K.EDGES for d in range(-1, 20) for f in (K.F19, K.F11) for last in (True, False)}
    assert {sep % K.LANE for sep, _, _ in seen} == set(range(K.LANE))
    assert any(sep - len(f) < E <= sep for sep, f, _ in seen for E in K.EDGES)                    # the field straddles the edge


def test_family_b_puts_the_boundary_on_the_stated_byte():
    seen = set()
    for (data, off, files), boundary, n_next in K.family_b():
        assert off[len(files) - 1 - n_next] == boundary and files[-1] == K.TAIL
        assert len(files[len(files) - 2 - n_next]) > 0                                            # a strict file ends at the boundary
        seen.add(boundary)
    assert seen == {E + d for E in K.EDGES for d in range(-17, 18)}


def test_family_c_has_a_lane_with_separators_of_two_files():
    data, off, files = K.family("C")[0]
    assert all(len(f) == 11 for f in files) and len(files) == 200 and len(set(files)) == 200
    file_of = [i for i, f in enumerate(files) for _ in f]
    lanes = {}
    for pos, c in enumerate(data):
        if c in SEPS:
            lanes.setdefault(pos // K.LANE, set()).add(file_of[pos])
    assert max(len(v) for v in lanes.values()) == 2
    data, off, files = K.family("C")[6]                                                           # 16-byte files: a boundary on every lane edge
    assert all(len(f) == K.LANE for f in files) and all(o % K.LANE == 0 for o in off)
    assert any(len(files) == 5 and not data for data, off, files in K.family("C"))


def test_family_d_puts_the_boundary_on_every_lane_residue():
    seen = {}
    for (data, off, files), boundary, pair in K.family_d():
        assert off[-3] == boundary and files[-3] == K.D_PAIRS[pair][0] and files[-2] == K.D_PAIRS[pair][1]
        seen.setdefault(pair, []).append(boundary)
    for pair, bs in seen.items():
        assert {b % K.LANE for b in bs if b != K.TILE} == set(range(K.LANE)) and K.TILE in bs


def test_family_e_declines_what_it_means_to():
    for kind in K.E_KINDS:
        for k in K.E_SEPS:
            f = K.declined(kind, k)
            assert R.classify(f) is None and sum(f.count(s) for s in (b",", b";")) == k + (kind == "semisemi")
    assert len(K.declined("stray", 700)) > 4 * K.TILE


def test_family_h_sizes():
    fam = K.family("H")
    assert {len(b[0]) for b in fam} >= {s + e for s in (K.LANE, K.TILE, K.WG) for e in (-1, 0, 1)}
    assert {len(b[2]) for b in fam} >= {255, 256, 257, 1023, 1024, 1025}
    data, off, files = K.big_batch()
    assert 1024 * K.TILE < len(data) <= 1026 * K.TILE and off[-3] > 1 << 20 and R.expect(files[-2], False) == R.HOST
    assert sum(len(f) > 100_000 for f in files) >= 3 and sum(len(f) < 100 for f in files) >= 300
