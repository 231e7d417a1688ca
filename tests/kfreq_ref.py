"""Test oracle for `poregen kmer_freq`: what the reference's subtool prints, restated in plain Python.

Lines are split the way getline(3) splits them: each ends after a newline byte, and a last line without one still counts. Lines are
numbered from 0; those whose number leaves remainder 1 when divided by 4 hold the sequence. From every such line its final byte is
removed (the newline, or, on an unterminated last line, a real byte) and every run of k consecutive bytes of what is left is a key.
Keys are byte strings: anything other than A, C, G, T is kept as it is. The printed table holds all 4^k ACGT strings (count 0 if never
seen) and every other key met, ordered by unsigned byte comparison unless a sort is asked for.
"""
import itertools
from collections import Counter


class NulInSequence(ValueError):
    """A sequence line holds a zero byte: the product refuses such input."""


def getline_split(data: bytes):
    out, start = [], 0
    while start < len(data):
        j = data.find(b"\n", start)
        end = len(data) if j < 0 else j + 1
        out.append(data[start:end])
        start = end
    return out


def count(data: bytes, k: int) -> Counter:
    c = Counter()
    for i, line in enumerate(getline_split(data)):
        if i % 4 != 1:
            continue
        body = line[:-1]
        content = line[:-1] if line.endswith(b"\n") else line
        if b"\0" in content:
            raise NulInSequence(i)
        for j in range(len(body) - k + 1):
            c[body[j:j + k]] += 1
    return c


def generated(k: int):
    return [bytes(t) for t in itertools.product(b"ACGT", repeat=k)]


def table(data: bytes, k: int):
    """[(key, count)] in byte order: the generated keys merged with every key that was met."""
    c = count(data, k)
    for key in generated(k):
        c.setdefault(key, 0)
    return sorted(c.items())


def render(entries, sort: int = 0, print_absent: int = 1) -> bytes:
    e = list(entries)
    if sort == 1:
        e.sort(key=lambda t: (t[1], t[0]))
    elif sort == 2:
        e.sort(key=lambda t: (t[1], t[0]), reverse=True)
    return b"".join(b"%s\t%d\n" % (key, n) for key, n in e if print_absent or n)


def expected(data: bytes, k: int, sort: int = 0, print_absent: int = 1) -> bytes:
    if not print_absent:  # the generated keys that were never met would be dropped anyway
        return render(sorted(count(data, k).items()), sort, 0)
    return render(table(data, k), sort, print_absent)
