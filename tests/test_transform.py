"""`poregen transform` (STEP 7 of scripts/poregen.sh: apply_transformation, set_stddev) on the host. The level_mean column is pinned to the
reference's own finished model (tests/golden/transform/poregen_5mer.model, a copy of its test/data/poregen_5mer.model): with the README's two
constants every one of its 1 024 texts comes back byte for byte, the 13 whose product has 21 decimals included. Everything else -- bc's
scale and truncation rules, the printing, the level_stdv projection, set_stddev, the refusals -- is checked against tests/bc_ref.py.
Host only: nothing here needs a GPU."""
import itertools
import os
import random
import subprocess
from fractions import Fraction

import pytest

import bc_ref
from poregen_amd.engine import transform_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("PG_REFORM_BIN") or os.path.join(ROOT, "bin", "poregen")  # PG_REFORM_BIN: the sanitizer build of the host-only subtools
FIXTURE = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")
A, B = "17.569300789355", "84.112089074928"  # README "Example workflow", STEP 7


def cli(*args):
    return subprocess.run([BIN, "transform"] + [str(a) for a in args], capture_output=True, timeout=120)


def dec_text(v, d):
    """the Fraction v, a multiple of 10^-d, written with d decimals"""
    n = abs(v) * 10 ** d
    assert n.denominator == 1
    digits = str(n.numerator).rjust(d + 1, "0")
    return ("-" if v < 0 else "") + (digits[:-d] + "." + digits[-d:] if d else digits)


def kmers(k, alphabet="ACGT"):
    return ["".join(t) for t in itertools.product(alphabet, repeat=k)]


def both(tmp_path, raw, *consts, stdv_from=None):
    """the model through the CLI (-o) and through engine.transform_model: the same bytes"""
    p = tmp_path / "raw_model"
    p.write_bytes(raw.encode())
    args = []
    if stdv_from is not None:
        (tmp_path / "from.model").write_bytes(stdv_from.encode())
        args = ["--stdv_from", tmp_path / "from.model"]
    for name, v in zip(("--stdv", "--mean", "--stdv_min", "--stdv_max"), consts):
        args += [name, v]
    r = cli(*args, "-o", tmp_path / "out.model", p)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-2000:]
    out = (tmp_path / "out.model").read_bytes().decode()
    assert cli(*args, p).stdout.decode() == out                       # stdout without -o
    assert transform_model(raw, *consts, stdv_from=stdv_from) == out
    return out


# ---- 1. the reference's file ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def recovered():
    """(fixture lines, raw medians, decimals needed): the raw median of every row of the reference's model, recovered from its level_mean"""
    lines = open(FIXTURE).read().split("\n")
    assert lines[-1] == "" and len(lines) == 7 + 1024 + 1
    a, b = Fraction(A), Fraction(B)
    medians, decimals = [], []
    for ln in lines[7:-1]:
        want = ln.split("\t")[1]
        x = (Fraction(want) - b) / a
        for d in range(15):
            text = dec_text(Fraction(round(x, d)), d)
            if bc_ref.level_mean(text, A, B) == want:
                medians.append(text); decimals.append(d)
                break
    return lines, medians, decimals


def test_reference_model_level_means(tmp_path, recovered):
    lines, medians, decimals = recovered
    assert len(medians) == 1024                                       # every row inverts
    assert sum(d == 9 for d in decimals) >= 10                        # means of two middle values: 21 decimals, truncated to 20
    assert max(decimals) == 9
    rng = random.Random(7)
    stdv = ["%.*f" % (rng.randint(1, 6), rng.uniform(0.9, 3.0)) for _ in medians]
    stdv[0], stdv[5], stdv[40] = "3.1", "0.625", "0.6250"             # AAAAA holds the largest, two rows the smallest
    names = [ln.split("\t")[0] for ln in lines[7:-1]]
    raw = "".join(f"{k}\t{m}\t{s}\n" for k, m, s in zip(names, medians, stdv))
    out = both(tmp_path, raw, A, B).split("\n")
    assert out[:7] == lines[:7]
    assert [ln.split("\t")[:2] for ln in out[7:]] == [ln.split("\t")[:2] for ln in lines[7:]]
    col = [ln.split("\t")[2] for ln in out[7:-1]]
    assert col[0] == "4.00000000000000000000" == lines[7].split("\t")[2]
    assert col[5] == col[40] == "2.50000000000000000000"
    assert "\n".join(out) == bc_ref.transform(raw, A, B)


# ---- 2. the rules against bc_ref -------------------------------------------------------------------------------------------

CONSTS = [
    (A, B, "2.5", "4"),
    ("1.234567890123456", "-.5", "2.125", "4.375"),   # A with 15 decimals, C / D with 3
    (".001", "0", "-1.5", "1"),                       # |level_mean| < 1, a level_stdv range across zero
    ("-3.25", "100.", "4", "2.5"),                    # negative A, D < C
]


def random_model(k, seed):
    rng = random.Random(seed)
    names = kmers(k)
    n = len(names)
    med, sd = [], []
    for i in range(n):
        d = rng.choice([0, 1, 3, 6, 9, 10, 12, 14])
        v = Fraction(rng.randint(-250 * 10 ** d, 250 * 10 ** d), 10 ** d)
        med.append(dec_text(v, d))
        d = rng.choice([1, 2, 6, 13, 18, 19])                       # 18 and 19 decimals: (s - min) * (D - C) has more than 20
        sd.append(dec_text(Fraction(rng.randint(16 * 10 ** (d - 1), 30 * 10 ** (d - 1)), 10 ** d), d))
    # the edges: trailing zeros as min and max, "5." and ".5", zero and minus zero, medians of 9 to 14 decimals of both signs
    med[0], med[1], med[2], med[3] = "-0.123456789", "97.12345678901234", "5.", "-.5"
    if n >= 16:
        med[4:10] = ["0", "-0", ".5", "-123.0000000001", "0.00000000000001", "-0.99999999999999"]
        sd[10], sd[11] = "2.", "3.0999999999999"
    sd[rng.randrange(n // 2)] = "1.50"
    sd[n // 2 + rng.randrange(n // 2)] = "3.10"
    return names, med, sd


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("consts", range(len(CONSTS)))
def test_rules_against_bc_ref(tmp_path, k, consts):
    names, med, sd = random_model(k, seed=100 * k + consts)
    raw = "".join(f"{a}\t{m}\t{s}\n" for a, m, s in zip(names, med, sd))
    if consts % 2:
        raw = raw[:-1]                                                # a last line without a newline counts
    want = bc_ref.transform(raw, *CONSTS[consts])
    assert both(tmp_path, raw, *CONSTS[consts]) == want
    assert want.count("\n") == 7 + 4 ** k and f"#k\t{k}\n" in want
    if consts == 2:
        col = [ln.split("\t")[1] for ln in want.split("\n")[7:-1]]
        assert all(not t.lstrip("-").startswith("0.") for t in col) and any(t.startswith("-.") for t in col) and any(t.startswith(".") for t in col)
        if k >= 2:
            assert col[4] == col[5] == "0"


def test_truncation_is_toward_zero_for_both_signs():
    """a product of scale 23 whose dropped digits are 889: no rounding up, in either direction"""
    raw = "AA\t0.33333333333\t1\nAC\t-0.33333333333\t2\n"
    out = transform_model(raw, "0.333333333333", "0", "0", "1").split("\n")
    assert out[7] == "AA\t.11111111110988888888\t0" and out[8] == "AC\t-.11111111110988888888\t1.00000000000000000000"
    assert "\n".join(out) == bc_ref.transform(raw, "0.333333333333", "0", "0", "1")
    assert bc_ref.show(bc_ref.mul(bc_ref.parse("0.33333333333"), bc_ref.parse("0.333333333333"))) == ".11111111110988888888"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_long_operands(seed):
    """operands of several machine words: extremes of 14 significant digits (a divisor above 2^32), level_stdv texts of up to 45 decimals
    (the divisor is scaled up instead of the dividend), medians and A of up to 30 decimals"""
    rng = random.Random(seed)
    long_text = lambda lo, hi, d: dec_text(Fraction(rng.randint(lo * 10 ** d, hi * 10 ** d), 10 ** d), d)
    sd = [long_text(2, 3, rng.choice([5, 21, 22, 30, 45])) for _ in range(16)]
    sd[3], sd[12] = ("1.2345678901234", "3.0999999999999") if seed else ("1", "3")
    med = [long_text(-200, 200, rng.choice([9, 14, 21, 30])) for _ in range(16)]
    raw = "".join(f"{a}\t{m}\t{s}\n" for a, m, s in zip(kmers(2), med, sd))
    consts = (long_text(-20, 20, 30), long_text(-100, 100, 25), "2.125", "4.3750000000000000000001")
    assert transform_model(raw, *consts) == bc_ref.transform(raw, *consts)


def test_further_columns_are_ignored(tmp_path):
    raw = "A\t1.5\t2\t9\tx\nC\t2\t3\t\nG\t-1\t2.5\nT\t0\t2.25"
    assert both(tmp_path, raw, "2", "1") == bc_ref.transform("A\t1.5\t2\nC\t2\t3\nG\t-1\t2.5\nT\t0\t2.25\n", "2", "1")


# ---- 3. --stdv_from (set_stddev) -------------------------------------------------------------------------------------------

def test_stdv_from_is_positional_and_verbatim(tmp_path):
    names, med, sd = random_model(2, seed=5)
    raw = "".join(f"{a}\t{m}\t{s}\n" for a, m, s in zip(names, med, sd))
    texts = ["3.10", "1e-05", "abc", "", " 2 ", "-.5"] + [str(i) for i in range(10)]
    # a U model for a T model, its rows in another order, further columns, no newline at the end: paste pairs them by position
    other = bc_ref.HEADER % 2 + "\n".join(f"{a}\t0\t{t}\t7\t8" for a, t in zip(reversed(kmers(2, "ACGU")), texts))
    plain = both(tmp_path, raw, A, B).split("\n")
    out = both(tmp_path, raw, A, B, stdv_from=other)
    assert out == bc_ref.transform(raw, A, B, stdv_from=other)
    rows = out.split("\n")
    assert rows[:7] == plain[:7] and [r.split("\t")[:2] for r in rows[7:-1]] == [r.split("\t")[:2] for r in plain[7:-1]]
    assert [r.split("\t")[2] for r in rows[7:-1]] == texts


def test_stdv_from_with_another_row_count_is_refused(tmp_path):
    names, med, sd = random_model(2, seed=5)
    raw = tmp_path / "raw"
    raw.write_text("".join(f"{a}\t{m}\t{s}\n" for a, m, s in zip(names, med, sd)))
    out = tmp_path / "out"
    out.write_bytes(b"kept")
    for n in (15, 17, 0):
        other = tmp_path / "other"
        other.write_text(bc_ref.HEADER % 2 + "".join(f"{a}\t0\t1\n" for a in (kmers(2) + ["TT"])[:n]))
        r = cli("--stdv", A, "--mean", B, "--stdv_from", other, "-o", out, raw)
        assert r.returncode == 1 and r.stdout == b"" and b"rows" in r.stderr and out.read_bytes() == b"kept"
        with pytest.raises(ValueError, match="rows"):
            transform_model(raw.read_text(), A, B, stdv_from=other.read_text())
    r = cli("--stdv", A, "--mean", B, "--stdv_from", tmp_path / "missing", "-o", out, raw)
    assert r.returncode == 1 and out.read_bytes() == b"kept"


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------

GOOD = "AA\t1.5\t2\nAC\t2\t3\nAG\t-1\t2.5\nAT\t0\t2.25\n"
REFUSED = {
    "exponent": GOOD.replace("\t2.5\n", "\t1e-05\n"),
    "exponent_mean": GOOD.replace("\t-1\t", "\t1e-05\t"),
    "nan": GOOD.replace("\t2.5\n", "\tnan\n"),
    "inf": GOOD.replace("\t-1\t", "\tinf\t"),
    "plus": GOOD.replace("\t2.5\n", "\t+1\n"),
    "blank": GOOD.replace("\t2.5\n", "\t 2.5\n"),
    "lone_minus": GOOD.replace("\t-1\t", "\t-\t"),
    "lone_point": GOOD.replace("\t-1\t", "\t.\t"),
    "empty_stddev": GOOD.replace("\t2.5\n", "\t\n"),
    "empty_mean": GOOD.replace("\t-1\t", "\t\t"),
    "two_fields": GOOD.replace("AG\t-1\t2.5\n", "AG\t-1\n"),
    "one_field": GOOD.replace("AG\t-1\t2.5\n", "AG\n"),
    "empty_line": GOOD.replace("AG\t", "\nAG\t"),
    "two_lengths": GOOD.replace("AG\t", "AGA\t"),
    "equal_stddevs": "AA\t1.5\t2\nAC\t2\t2.0\nAG\t-1\t2.00\n",
    "one_row": "AA\t1.5\t2\n",
    "empty_file": "",
    "smallest_prints_an_exponent": GOOD.replace("\t2\n", "\t0.00001\n"),
    "line_of_70": GOOD.replace("\t-1\t", "\t" + "9" * 60 + "\t"),
    "crlf": GOOD.replace("\n", "\r\n"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_write_nothing(tmp_path, case):
    raw, out = tmp_path / "raw", tmp_path / "out.model"
    raw.write_bytes(REFUSED[case].encode())
    out.write_bytes(b"an earlier model\n")
    r = cli("--stdv", A, "--mean", B, "-o", out, raw)
    assert r.returncode == 1 and r.stdout == b"" and b"[transform::ERROR]" in r.stderr, r.stderr
    assert out.read_bytes() == b"an earlier model\n"
    assert cli("--stdv", A, "--mean", B, raw).stdout == b""
    if case not in ("empty_file", "equal_stddevs", "one_row", "smallest_prints_an_exponent"):
        assert b"line " in r.stderr                                   # the line is named
    if case in ("two_fields", "one_field"):
        assert b"line 3" in r.stderr and b"no samples" in r.stderr
    with pytest.raises(ValueError):
        transform_model(REFUSED[case], A, B)
    with pytest.raises(ValueError):
        bc_ref.transform(REFUSED[case], A, B)
    r = cli("--stdv", A, "--mean", B, "-o", out, raw.with_name("missing"))
    assert r.returncode == 1 and out.read_bytes() == b"an earlier model\n"


@pytest.mark.parametrize("bad", ["1e-05", "nan", "inf", "+1", "", "1,5"])
def test_constants_that_are_no_numbers(tmp_path, bad):
    raw, out = tmp_path / "raw", tmp_path / "out.model"
    raw.write_text(GOOD)
    out.write_bytes(b"kept")
    for args in (["--stdv", bad, "--mean", B], ["--stdv", A, "--mean", bad], ["--stdv", A, "--mean", B, "--stdv_min", bad],
                 ["--stdv", A, "--mean", B, "--stdv_max", bad]):
        r = cli(*args, "-o", out, raw)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr and out.read_bytes() == b"kept", args
    with pytest.raises(ValueError, match="--stdv"):
        transform_model(GOOD, bad, B)


def test_option_combinations(tmp_path):
    raw, out = tmp_path / "raw", tmp_path / "out.model"
    raw.write_text(GOOD)
    out.write_bytes(b"kept")
    for args in (["--signal", "reads.blow5", "--mean", B], ["--signal", "reads.blow5", "--stdv", A], ["--signal", "reads.blow5", "--stdv", A, "--mean", B],
                 [], ["--stdv", A], ["--mean", B], ["--no_such_option", "--stdv", A, "--mean", B]):
        r = cli(*args, "-o", out, raw)
        assert r.returncode == 1 and r.stdout == b"" and b"Usage: poregen transform" in r.stderr, args
        assert out.read_bytes() == b"kept"
    assert cli("--stdv", A, "--mean", B).returncode == 1              # no RAW_MODEL
    assert cli("--stdv", A, "--mean", B, raw, raw).returncode == 1    # two of them
    r = cli("-h")
    assert r.returncode == 0 and b"Usage: poregen transform" in r.stdout and b"--stdv_from" in r.stdout
    r = subprocess.run([BIN, "--help"], capture_output=True)
    assert r.returncode == 0 and b"transform" in r.stdout
