"""Inputs shared by the simulate tests (test_sim_host.py, test_gpu_sim.py): model tables, sequences, the reference's walk kept per read."""
import functools

import numpy as np

import sim_ref as S


@functools.lru_cache(maxsize=None)
def tables(k, seed=1, missing=(), dwell=None, stdv=None, level=None):
    """(levels, stdvs, dwells) of 4^k slots each: levels 50 to 130 pA, stdvs 0.5 to 4 pA, dwells 3 to 15 samples, unless one value is given
    for all; the slots in `missing` have no level."""
    rng = np.random.default_rng(seed)
    n = 4 ** k
    lv = rng.integers(50000, 130000, n).astype(np.uint32) if level is None else np.full(n, level, np.uint32)
    sd = rng.integers(500, 4000, n).astype(np.uint32) if stdv is None else np.full(n, stdv, np.uint32)
    dw = rng.integers(3, 16, n).astype(np.uint32) if dwell is None else np.full(n, dwell, np.uint32)
    for s in missing:
        lv[s] = 0
    for a in (lv, sd, dw):
        a.flags.writeable = False
    return lv, sd, dw


def rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


_WALKS = {}


def expected(R, tab, tab_id, seq, read):
    """sim_ref.walk, computed once per (rule, tables, read)."""
    key = (repr(R), tab_id, seq, read)
    if key not in _WALKS:
        _WALKS[key] = S.walk(R, tab[0], tab[1], tab[2], seq, read)
    return _WALKS[key]


def edge_lengths(k):
    """Bases per read: around k, and around the step of 64 ops and the piece of 256."""
    return [1, max(k - 1, 1), k, k + 1, 63, 64, 65, 255, 256, 257, 1025]
