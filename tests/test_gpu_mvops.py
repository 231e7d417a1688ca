"""pg_mvops_expand on the MI355X, through poregen_amd.engine.MoveExpander / reform_ops: move tables at the edges of the kernels' shapes
(the 64 elements of a ballot, the 16-byte loads and their misaligned ends, the piece of a long read) against tests/mvops_ref.py, the
Python restatement of `poregen reform -c -k 1 -m 0` that the reference's goldens pin (tests/test_mvops_host.py). Element for element:
ops, op_off, the three scalars, seq, seq_off, statuses. The piece size comes from the library."""
import numpy as np
import pytest

import mvops_cases as M
import mvops_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from poregen_amd.engine import MoveExpander
    e = MoveExpander()
    yield e
    e.close()


@pytest.fixture(scope="module")
def edge(ex):
    assert ex.piece >= 1024 and ex.piece % 1024 == 0
    return M.edge_reads(ex.piece)


def run(ex, reads, flags=0, device=False, **lay):
    a = M.layout(reads, **lay)
    if device:
        import torch
        a = {k: torch.from_numpy(v.copy()).cuda() for k, v in a.items()}
    return ex.expand(a["mv"], a["mv_off"], a["stride"], a["ns"], a["ts"], a["l_seq"], a["flag"], a["seq_bytes"], a["byte_off"],
                     rna=bool(flags & R.RNA), n_to_t=bool(flags & R.N_TO_T))


def same(res, reads, flags=0):
    want = M.expected(reads, flags)
    got = res.to_host()
    assert np.array_equal(res.status, want["status"]) and np.array_equal(got["status"], want["status"])
    for key in ("op_off", "seq_off", "op_n", "seq", "target_start", "target_end"):
        assert np.array_equal(got[key], want[key]), key
    ok = want["status"] == R.OK
    assert np.array_equal(got["query_start"][ok], want["query_start"][ok])
    assert res.n_ops == int(want["op_off"][-1]) == got["op_t"].size and not got["op_t"].any()
    refused = np.flatnonzero(~ok)
    assert res.n_refused == refused.size and res.first_refused == (int(refused[0]) if refused.size else -1)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("flags", [0, R.RNA, R.N_TO_T, R.RNA | R.N_TO_T])
def test_every_edge_read_in_one_batch(ex, edge, flags, device):
    reads = [r for _, r in edge]
    same(run(ex, reads, flags, device), reads, flags)


def test_every_edge_read_alone(ex, edge):
    for label, r in edge:
        same(run(ex, [r]), [r])
        same(run(ex, [r], device=True, lead=5), [r])


@pytest.mark.parametrize("device", [False, True])
def test_tables_at_every_byte_alignment(ex, device):
    reads = M.alignment_reads()
    for lead in range(16):                                   # ... and the first table at every offset of the array itself
        same(run(ex, reads, lead=lead, seq_gaps=(0, 1, 3), seq_lead=lead % 3, device=device), reads)


def test_device_arrays_at_unaligned_pointers(ex, edge):
    import torch
    reads = [r for _, r in edge][:30]
    a = M.layout(reads)
    for shift in (1, 7, 13):
        mv = torch.from_numpy(np.concatenate([np.ones(shift, np.int8), a["mv"]])).cuda()[shift:]
        sq = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), a["seq_bytes"]])).cuda()[shift:]
        t = {k: torch.from_numpy(v.copy()).cuda() for k, v in a.items() if k not in ("mv", "seq_bytes")}
        res = ex.expand(mv, t["mv_off"], t["stride"], t["ns"], t["ts"], t["l_seq"], t["flag"], sq, t["byte_off"])
        same(res, reads)


def test_batch_whose_last_read_is_refused_and_empty_batch(ex, edge):
    cases = dict(edge)
    reads = [cases["n129"], cases["stride10"], cases["fewer_moves_than_bases"]]
    res = run(ex, reads)
    same(res, reads)
    assert res.first_refused == 2 and res.n_refused == 1 and res.status[2] == R.BASES_LEFT
    res = run(ex, [])
    assert res.n_reads == 0 and res.n_ops == 0 and res.first_refused == -1 and res.op_off.cpu().tolist() == [0]


def test_reverse_and_n_by_hand(ex):
    import kfreq_reads_cases as K
    rd = M.Rd([1, 0, 1, 0, 1, 1, 0], 5, 60, 4, K.codes_of(b"ANAC"), flag=0x10)     # stored ANAC with flag 0x10 prints GTNT
    res = run(ex, [rd])
    h = res.to_host()
    assert bytes(h["seq"]) == b"GTNT" and list(h["op_n"]) == [10, 10, 5, 5 + (60 - (6 * 5 + 4))] and list(h["query_start"]) == [4]
    assert bytes(run(ex, [rd], R.N_TO_T).to_host()["seq"]) == b"GTTT"
    h = run(ex, [rd], R.RNA).to_host()
    assert (list(h["target_start"]), list(h["target_end"])) == ([4], [0])


def test_many_reads_and_one_shot(ex):
    from poregen_amd.engine import reform_ops
    rng = np.random.default_rng(5)
    reads = [M.good(rng, M.table(rng, int(n), first=int(f)), stride=int(s), flag=0x10 if i % 5 == 0 else 0, n_rate=0.02)
             for i, (n, f, s) in enumerate(zip(rng.integers(1, 900, 3000), rng.integers(0, 3, 3000), rng.choice([5, 6, 10], 3000)))]
    same(run(ex, reads), reads)
    same(run(ex, reads, device=True), reads)
    a = M.layout(reads[:100])
    out = reform_ops(a["mv"], a["mv_off"], a["stride"], a["ns"], a["ts"], a["l_seq"], a["flag"], a["seq_bytes"], a["byte_off"], rna=True)
    want = M.expected(reads[:100], R.RNA)
    assert all(np.array_equal(out[k], want[k]) for k in ("op_n", "op_off", "seq", "seq_off", "status", "target_start", "target_end"))


def test_refused_layouts(ex, edge):
    from poregen_amd import _abi
    from poregen_amd.engine import PgError
    reads = [r for _, r in edge][:5]
    a = M.layout(reads)
    bad_off = a["mv_off"].copy(); bad_off[-1] += 1
    short_seq = a["seq_bytes"][:-1]
    for kw in (dict(mv_off=bad_off), dict(seq_bytes=short_seq)):
        b = dict(a); b.update(kw)
        with pytest.raises(PgError) as ei:
            ex.expand(b["mv"], b["mv_off"], b["stride"], b["ns"], b["ts"], b["l_seq"], b["flag"], b["seq_bytes"], b["byte_off"])
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG
    same(run(ex, reads), reads)                              # the handle stays usable
