"""pg_mvops_project_stranded on the MI355X, through poregen_amd.engine.MoveExpander.project(reverse=, contig_len=): the reads and CIGARs
of tests/refops_cases.py, each in both directions with the strands alternating along the batch, element for element against
tests/strand_ref.py -- which reduces a reverse read to the merged forward rule of tests/refops_ref.py. CIGARs of 1, 63, 64, 65 and 129
words, M runs across a piece edge, I runs summed by a lane, by the wave and longer than a piece, clips of 0, 1, 4096 and 5000 bases at the
end that becomes the front, batches of 0, 1 and 300 reads, host and device arrays, with and without PG_MVOPS_RNA, status 8 between accepted
neighbours; and without strands the call is pg_mvops_project."""
import numpy as np
import pytest

import refops_cases as X
import strand_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from poregen_amd.engine import MoveExpander
    e = MoveExpander()
    assert e.piece == X.P
    yield e
    e.close()


@pytest.fixture(scope="module")
def edge():
    return SC.edge_cases() + SC.rule_cases()


@pytest.fixture(scope="module")
def rand300():
    return SC.random_batch(300)


def up(a, view):
    import torch
    return torch.from_numpy(a.view(view).copy()).cuda()


def run(ex, cases, rna=False, device=False, cigar_lead=0, strands=True):
    a = SC.layout(cases, cigar_lead)
    ops = (up(a["op_n"], np.int32), up(a["op_off"], np.int64), up(a["query_start"], np.int32), up(a["status"], np.int32))
    cg = (up(a["cigar"], np.int32), up(a["cigar_off"], np.int64), up(a["pos"], np.int32)) if device else (a["cigar"], a["cigar_off"], a["pos"])
    st = {} if not strands else dict(reverse=up(a["reverse"], np.uint8), contig_len=up(a["contig_len"], np.int32)) if device else dict(reverse=a["reverse"], contig_len=a["contig_len"])
    return ex.project(ops, *cg, rna=rna, **st)


def same(res, cases, rna=False):
    want = SC.expected(cases, rna)
    got = res.to_host()
    for key in ("status", "op_off", "op_n", "op_t", "query_start", "query_end", "target_start", "target_end", "ref_len", "n_match"):
        assert np.array_equal(got[key], want[key]), (key, [c.label for c, a, b in zip(cases, got[key], want[key]) if key not in ("op_n", "op_t", "op_off") and a != b][:5])
    assert np.array_equal(res.status, want["status"]) and np.array_equal(res.ref_len_host, want["ref_len"])
    assert np.array_equal(res.n_match_host, want["n_match"]) and np.array_equal(res.query_end_host, want["query_end"])
    assert res.n_ops == int(want["op_off"][-1]) == got["op_t"].size
    refused = np.flatnonzero(want["status"] != 0)
    assert res.n_refused == refused.size and res.first_refused == (int(refused[0]) if refused.size else -1)


def test_the_cases_hold_what_the_kernels_can_get_wrong(edge):
    by = {c.label: c for c in edge}
    for n in (1, 63, 64, 65, 129):
        assert len(by[f"words{n}-"].words) == n and by[f"words{n}-"].reverse and not by[f"words{n}+"].reverse
    for label in ("m_across_piece_edge-", "i1-", "i64-", "i70-", "i_longer_than_a_piece-", "trailing_s-", "trailing_s_long-", "lead_s0-", "lead_s1-", f"lead_s{X.P}-", "lead_s5000-"):
        assert by[label].ref().status == 0
    # a trailing clip of the stored CIGAR is the leading clip of a reverse DNA read: it moves query_start
    c = by["trailing_s_long-"]
    assert c.ref().query_start == c.qs + sum(c.o[:X.P + 5]) and by["trailing_s_long+"].ref().query_start == c.qs
    st = [c.ref().status for c in SC.rule_cases()]
    assert st[:5] == [0, 8, 0, 8, 0]                        # status 8 between accepted neighbours


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("rna", [False, True])
def test_every_edge_case_in_one_batch(ex, edge, rna, device):
    same(run(ex, edge, rna, device, cigar_lead=3 if device else 0), edge, rna)


@pytest.mark.parametrize("rna", [False, True])
def test_reverse_edge_cases_alone(ex, edge, rna):
    for c in edge:
        if c.reverse:
            same(run(ex, [c], rna), [c], rna)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("rna", [False, True])
def test_batches_of_0_1_and_300_reads(ex, rand300, rna, device):
    res = run(ex, [], rna, device)
    assert res.n_reads == 0 and res.n_ops == 0 and res.first_refused == -1 and res.op_off.cpu().tolist() == [0]
    same(run(ex, rand300[1:2], rna, device), rand300[1:2], rna)
    assert rand300[1].reverse and [c.reverse for c in rand300[:4]] == [False, True, False, True]
    same(run(ex, rand300, rna, device), rand300, rna)


@pytest.mark.parametrize("rna", [False, True])
def test_without_strands_it_is_pg_mvops_project(ex, rand300, rna):
    """strands == NULL (project without the two arrays), and a pg_mvops_strands whose pointers are NULL, against pg_mvops_project; all
    reads forward gives the same again."""
    import ctypes as C
    import torch
    from poregen_amd import _abi
    from poregen_amd.engine import RefOps
    cases = rand300[:80] + SC.edge_cases()[:40]
    a = SC.layout(cases)
    plain = run(ex, cases, rna, strands=False).to_host()
    fwd = [SC.SCase(c, False, 0) for c in cases]
    got = run(ex, fwd, rna).to_host()
    for key in plain:
        assert np.array_equal(plain[key], got[key]), key
    assert np.array_equal(plain["status"], X.expected(cases, rna)["status"])   # the merged rule: no strand looked at
    ops = (up(a["op_n"], np.int32), up(a["op_off"], np.int64), up(a["query_start"], np.int32), up(a["status"], np.int32))
    c = _abi.PgMvopsCigars()
    c.n_reads, c.location, c.flags = len(cases), _abi.PG_LOC_HOST, (_abi.PG_MVOPS_RNA if rna else 0)
    c.op_n, c.n_ops, c.op_off, c.query_start, c.status = ops[0].data_ptr(), ops[0].numel(), ops[1].data_ptr(), ops[2].data_ptr(), ops[3].data_ptr()
    c.cigar, c.n_cigar, c.cigar_off, c.pos = a["cigar"].ctypes.data, a["cigar"].size, a["cigar_off"].ctypes.data, a["pos"].ctypes.data
    for strands in (None, C.byref(_abi.PgMvopsStrands())):
        res = _abi.PgMvopsProjection()
        assert ex._lib.pg_mvops_project_stranded(ex._h, C.byref(c), strands, C.byref(res)) == 0
        got = RefOps(res, ex.device).to_host()
        for key in plain:
            assert np.array_equal(plain[key], got[key]), key
    torch.cuda.synchronize()


def test_refused_arguments(ex, rand300):
    from poregen_amd import _abi
    from poregen_amd.engine import PgError
    import ctypes as C
    cases = rand300[:6]
    a = SC.layout(cases)
    ops = (up(a["op_n"], np.int32), up(a["op_off"], np.int64), up(a["query_start"], np.int32), up(a["status"], np.int32))
    with pytest.raises(ValueError):
        ex.project(ops, a["cigar"], a["cigar_off"], a["pos"], reverse=a["reverse"])
    with pytest.raises(ValueError):
        ex.project(ops, a["cigar"], a["cigar_off"], a["pos"], reverse=up(a["reverse"], np.uint8), contig_len=a["contig_len"])
    with pytest.raises(ValueError):
        ex.project(ops, a["cigar"], a["cigar_off"], a["pos"], reverse=a["reverse"][:3], contig_len=a["contig_len"])
    # one of the two pointers alone
    c = _abi.PgMvopsCigars()
    c.n_reads, c.location = len(cases), _abi.PG_LOC_HOST
    c.op_n, c.n_ops, c.op_off, c.query_start, c.status = ops[0].data_ptr(), ops[0].numel(), ops[1].data_ptr(), ops[2].data_ptr(), ops[3].data_ptr()
    c.cigar, c.n_cigar, c.cigar_off, c.pos = a["cigar"].ctypes.data, a["cigar"].size, a["cigar_off"].ctypes.data, a["pos"].ctypes.data
    s = _abi.PgMvopsStrands()
    s.reverse = a["reverse"].ctypes.data
    res = _abi.PgMvopsProjection()
    assert ex._lib.pg_mvops_project_stranded(ex._h, C.byref(c), C.byref(s), C.byref(res)) == _abi.PG_ERR_INVALID_ARG
    # device CIGARs with host strands
    with pytest.raises(PgError) as ei:
        s.contig_len = a["contig_len"].ctypes.data
        c.location = _abi.PG_LOC_DEVICE
        dc = (up(a["cigar"], np.int32), up(a["cigar_off"], np.int64), up(a["pos"], np.int32))
        c.cigar, c.cigar_off, c.pos = dc[0].data_ptr(), dc[1].data_ptr(), dc[2].data_ptr()
        st = ex._lib.pg_mvops_project_stranded(ex._h, C.byref(c), C.byref(s), C.byref(res))
        raise PgError(st, ex._lib.pg_mvops_last_error(ex._h).decode())
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "device memory" in str(ei.value)
    same(run(ex, cases), cases)                              # the handle stays usable
