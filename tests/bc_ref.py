"""What `bc -l` (scale = 20) and STEP 7 of scripts/poregen.sh (apply_transformation, set_stddev) compute, restated with
fractions.Fraction -- independent of csrc/pg_bcdec.h and pg_transform.h, for tests/test_transform.py and test_gpu_transform.py.

A number is (value: Fraction, scale: int); the value is always a multiple of 10^-scale.
  parse   -?D*(.D*)? with at least one digit; scale = digits behind the point
  + -     exact, scale max(sa, sb)
  *       scale min(sa + sb, max(20, sa, sb)), truncated toward zero
  /       scale 20, truncated toward zero
  print   all digits of the scale, no zero before the point, zero prints "0"; bc breaks a line after 69 characters, the tool refuses
          a text of more than 68
"""
import re
from decimal import ROUND_HALF_EVEN, Context
from fractions import Fraction

SCALE = 20
NUMBER = re.compile(r"-?[0-9]*(\.[0-9]*)?\Z")
HEADER = ("#ont_model_name\tnone\n#kit\tnone\n#strand\ttemplate\n#k\t%d\n#alphabet\tnucleotide\n#original_file\tnone\n"
          "kmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\tweight\n")


def is_number(text):
    return bool(NUMBER.match(text)) and any(ch.isdigit() for ch in text)


def parse(text):
    if not is_number(text):
        raise ValueError(f"not a number to bc: {text!r}")
    frac = text.partition(".")[2]
    body = text.lstrip("-")
    v = Fraction(int(body.replace(".", "") or "0"), 10 ** len(frac))
    return (-v if text.startswith("-") else v, len(frac))


def _trunc(v, scale):
    """v cut to `scale` decimals, toward zero"""
    n = abs(v) * 10 ** scale
    q = n.numerator // n.denominator
    return Fraction(q if v >= 0 else -q, 10 ** scale)


def add(a, b):
    return (a[0] + b[0], max(a[1], b[1]))


def sub(a, b):
    return (a[0] - b[0], max(a[1], b[1]))


def mul(a, b):
    s = min(a[1] + b[1], max(SCALE, a[1], b[1]))
    return (_trunc(a[0] * b[0], s), s)


def div(a, b):
    if b[0] == 0:
        raise ZeroDivisionError("divide by zero")
    return (_trunc(a[0] / b[0], SCALE), SCALE)


def show(a):
    v, s = a
    if v == 0:
        return "0"
    n = abs(v) * 10 ** s
    assert n.denominator == 1
    digits = str(n.numerator).rjust(s, "0")
    ip, fp = (digits[:-s], digits[-s:]) if s else (digits, "")
    return ("-" if v < 0 else "") + ip + ("." + fp if s else "")


def datamash_g(text):
    """`datamash min 1 max 1` prints "%.14Lg" of the value: at most 14 significant digits, trailing zeros gone. (A text of 15 digits or
    more is rounded to even here on its exact value; the tests stay below that, where nothing is rounded.)"""
    d = Context(prec=14, rounding=ROUND_HALF_EVEN).create_decimal(text)
    if d == 0:
        return "-0" if d.is_signed() else "0"
    if not -4 <= d.adjusted() < 14:
        raise ValueError("%.14Lg prints an exponent: not a number to bc")
    t = format(d, "f")
    return t.rstrip("0").rstrip(".") if "." in t else t


def level_mean(median, A, B):
    return show(add(mul(parse(median), parse(A)), parse(B)))


def transform(raw_text, A, B, C="2.5", D="4", stdv_from=None):
    """the model file of a raw model text, or ValueError where poregen transform refuses"""
    lines = raw_text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if not lines:
        raise ValueError("empty model")
    rows = []
    for ln in lines:
        f = ln.split("\t")
        if len(f) < 3:
            raise ValueError("no samples")
        if len(f[0]) != len(lines[0].split("\t")[0]) or not f[0]:
            raise ValueError("k-mer length")
        rows.append((f[0], parse(f[1]), parse(f[2]), f[2]))
    a, b, c, d = parse(A), parse(B), parse(C), parse(D)
    mn = parse(datamash_g(min(rows, key=lambda r: r[2][0])[3]))
    mx = parse(datamash_g(max(rows, key=lambda r: r[2][0])[3]))
    span = sub(mx, mn)
    if span[0] == 0:
        raise ValueError("max == min")
    col = None
    if stdv_from is not None:
        fl = stdv_from.split("\n")
        if fl and fl[-1] == "":
            fl.pop()
        col = [ln.split("\t")[2] for ln in fl[7:]]
        if len(col) != len(rows):
            raise ValueError("row counts differ")
    out = [HEADER % len(rows[0][0])]
    for i, (kmer, m, s, _) in enumerate(rows):
        mean = show(add(mul(m, a), b))
        stdv = show(add(div(mul(sub(s, mn), sub(d, c)), span), c))
        if max(len(mean), len(stdv)) > 68:
            raise ValueError("bc would break the line")
        out.append(f"{kmer}\t{mean}\t{col[i] if col is not None else stdv}\n")
    return "".join(out)
