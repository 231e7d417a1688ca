"""The dump-text parser of `poregen model` (pg_dumptext.hip) on the seams of its decomposition: the batches of tests/dumptext_cases.py
through engine.DumpModel against tests/dumptext_ref.py (Python integers; tied to oracle/model_oracle.c and to the field rule by
tests/test_dumptext_host.py). Files the reference gives to the host must be exactly the handle's host files, with the oracle's texts."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dumptext_cases as K
import dumptext_ref as R
from poregen_amd import _abi
from poregen_amd.engine import DumpModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle", "model_oracle")
GUARD = b";1.00000000;"       # around device bytes: a read outside the batch would change a count
FIRST = b"9.00000000,"        # in front of a file for the oracle, whose `tail -n +2` drops it: the oracle's texts with the first value kept

expect = functools.lru_cache(maxsize=None)(R.expect)
_oracle_texts = {}            # (file bytes, keep_first) -> (median, stddev capped at 1e9, dwell) as model_oracle prints them


def _columns(mode, d, *args):
    out = subprocess.run([ORACLE, mode, d] + list(args), capture_output=True, check=True).stdout.decode()
    return [l.split("\t")[1:] for l in out.split("\n")[:-1]]


def oracle_texts(files, keep_first):
    """the oracle's three texts for each of the files, from one directory of those not seen before"""
    new = [f for f in dict.fromkeys(files) if (f, keep_first) not in _oracle_texts]
    if new:
        with tempfile.TemporaryDirectory(prefix="pg_dt") as tmp:
            for sub, lead in (("plain", b""), ("first", FIRST)):
                os.mkdir(os.path.join(tmp, sub))
                for i, f in enumerate(new):
                    with open(os.path.join(tmp, sub, "f%06d" % i), "wb") as fh:
                        fh.write(lead + f)
            stats = _columns("stats", os.path.join(tmp, "first" if keep_first else "plain"), "1e9")
            dwell = _columns("dwell", os.path.join(tmp, "plain"))
        for f, (med, sd), (dw,) in zip(new, stats, dwell):
            _oracle_texts[(f, keep_first)] = (med, sd, dw)
    return [_oracle_texts[(f, keep_first)] for f in files]


def capped(sd, limit="1e9"):
    return limit if sd not in ("", "nan") and float(sd) > float(limit) else sd


def host_bytes(b):
    return b[0]


def run(dm, batches, data_of=host_bytes):
    for b in batches:
        dm.submit(data_of(b), b[1])
    return dm.finish()


def check(dm, batches, keep_first, data_of=host_bytes):
    """the batches through one handle and one finish(): every file against the reference, the host files against the oracle"""
    m, info = run(dm, batches, data_of)
    files = [f for b in batches for f in b[2]]
    want = [expect(f, keep_first) for f in files]
    assert info.n_files == len(files) == len(m.n_values) and info.n_bytes == sum(len(b[0]) for b in batches)
    assert [int(i) for i in info.host_files] == [i for i, e in enumerate(want) if e == R.HOST]
    assert info.n_host_files == len(info.host_files)
    assert info.n_values == sum(R.parsed_values(f) for f in files)
    for i, e in enumerate(want):
        if e == R.HOST:
            continue
        got = (int(m.n_values[i]), int(m.mid_lo[i]), int(m.mid_hi[i]), int(m.origin[i]), int(m.sum1[i]), (int(m.sum2_hi[i]) << 64) + int(m.sum2_lo[i]),
               int(m.dwell_n[i]), float(m.dwell_median[i]) if e.dwell_n else None)
        assert got == tuple(e), (i, files[i][:80], got, e)
    host = [i for i, e in enumerate(want) if e == R.HOST]
    for i, (med, sd, dw) in zip(host, oracle_texts([files[i] for i in host], keep_first)):
        assert (m.median_text[i], capped(m.sstdev_text[i]), m.dwell_text[i]) == (med, sd, dw), (i, files[i][:80])
    return m, info


def records(m, info):
    """everything the handle says per file, for comparing two runs"""
    host = set(int(i) for i in info.host_files)
    cols = [m.n_values, m.mid_lo, m.mid_hi, m.origin, m.sum1, m.sum2_lo, m.sum2_hi, m.dwell_n]
    return [tuple(int(c[i]) for c in cols) + (m.median_text[i], m.sstdev_text[i], m.dwell_text[i], i in host) for i in range(len(m.n_values))]


def device_bytes(shift):
    """data_of: the batch's bytes as a view `shift` bytes into a CUDA tensor, guard text in front of it and behind it"""
    import torch

    def data_of(b):
        buf = (GUARD * 3)[len(GUARD) * 3 - shift:] + b[0] + GUARD * 6
        t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        assert t.data_ptr() % 16 == 0
        return t[shift:shift + len(b[0])]
    return data_of


@pytest.mark.parametrize("keep_first", [False, True], ids=["tail", "keep_first"])
@pytest.mark.parametrize("name", list(K.FAMILIES))
def test_family(name, keep_first):
    dm = DumpModel(keep_first=keep_first)
    fam = K.family(name)
    check(dm, fam, keep_first)
    check(dm, fam[::-1][:40], keep_first)          # the handle again, its buffers grown: other batches meet in the two slots
    dm.close()


@pytest.mark.parametrize("shift", [16, 1, 7, 8, 15])
def test_device_bytes(shift):
    """one batch of every family read in place: shift 16 is a 16-byte aligned view (the kAligned kernels), the others are not. The same
    results as from host bytes, the files the device declines -- copied back for the host path -- and their texts included."""
    batches = [K.representative(name) for name in K.FAMILIES]
    for keep_first in (False, True):
        dm = DumpModel(keep_first=keep_first)
        want = records(*check(dm, batches, keep_first))
        got = records(*check(dm, batches, keep_first, device_bytes(shift)))
        dm.close()
        assert got == want
        assert sum(r[-1] for r in want) >= 5


def slot_batches():
    small1 = K.batch([K.pad(300), K.declined("plus", 1), K.pad(40)])
    large = K.batch([K.pad(150_000, seed=1), K.declined("int9", 70), K.pad(150_000, seed=2), K.TAIL])
    small2 = K.representative("E")
    medium = K.batch([K.pad(20_000), K.declined("stray", 700), K.pad(9_000), K.declined("no_final", 1)])
    return [small1, large, small2, medium], [False, True, True, False]


def test_slots():
    """small (host), large (device: the buffers grow while the small one is in flight), small (device), medium (host) through one handle:
    the results of each batch run alone, in submission order; a submit without files changes nothing; finish() forgets"""
    batches, on_device = slot_batches()
    dev = device_bytes(7)
    device_ids = {id(b) for b, d in zip(batches, on_device) if d}
    data_of = lambda b: dev(b) if id(b) in device_ids else b[0]
    alone = []
    for b in batches:
        dm = DumpModel()
        alone += records(*check(dm, [b], False, data_of))
        dm.close()
    dm = DumpModel()
    assert records(*check(dm, batches, False, data_of)) == alone
    for b in batches:                              # the same with empty submits in between
        dm.submit(data_of(b), b[1])
        dm.submit(b"", [0])
    m, info = dm.finish()
    assert records(m, info) == alone and info.n_files == sum(len(b[2]) for b in batches)
    m, info = run(dm, [batches[3]])                # after finish(): the old results are gone
    assert info.n_files == len(batches[3][2]) and records(m, info) == alone[-len(batches[3][2]):]
    dm.close()


def test_refused_submits_leave_the_pending_batch_intact():
    good1, good2 = K.representative("B"), K.representative("E")
    dm = DumpModel()
    want = records(*check(dm, [good1, good2], False))
    data = np.frombuffer(good2[0], np.uint8)
    submit = lambda off, n_files, loc: dm._lib.pg_dmodel_submit(dm._h, C.c_void_p(data.ctypes.data), C.c_void_p(off.ctypes.data), n_files, loc)
    dm.submit(good1[0], good1[1])
    assert submit(np.array([1, 12], np.uint64), 1, _abi.PG_LOC_HOST) == _abi.PG_ERR_INVALID_ARG
    assert submit(np.array([0, 12, 5], np.uint64), 2, _abi.PG_LOC_HOST) == _abi.PG_ERR_INVALID_ARG
    assert submit(np.array([0, 12], np.uint64), 1, 7) == _abi.PG_ERR_INVALID_ARG
    assert b"location" in dm._lib.pg_dmodel_last_error(dm._h)
    dm.submit(good2[0], good2[1])
    assert submit(np.array([1, 12], np.uint64), 1, _abi.PG_LOC_HOST) == _abi.PG_ERR_INVALID_ARG      # with both slots taken
    assert records(*dm.finish()) == want
    dm.close()


def test_more_than_1024_tiles():
    """1 MiB + 2 tiles: k_dt_scan takes two tiles per thread; host bytes and device bytes"""
    b = K.big_batch()
    assert len(b[0]) > 1024 * K.TILE
    dm = DumpModel()
    want = records(*check(dm, [b], False))
    assert records(*check(dm, [b], False, device_bytes(16))) == want
    assert records(*check(dm, [b], False, device_bytes(1))) == want
    dm.close()
