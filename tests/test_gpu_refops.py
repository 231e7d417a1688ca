"""pg_mvops_project on the MI355X, through poregen_amd.engine.MoveExpander.project / project_ops: reads and CIGARs at the edges of the rule
and of the kernels' shapes (the 64 words of a step, the piece of query bases, I runs summed by a lane or by the wave, clips, refusals)
against tests/refops_ref.py, the Python restatement of the rule. Element for element: ops, their types, op_off, the four scalars,
ref_len, n_match, statuses -- with and without PG_MVOPS_RNA, CIGAR arrays on the host and on the device."""
import numpy as np
import pytest

import mvops_cases as M
import mvops_ref as MR
import refops_cases as X

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
    return X.edge_cases()


@pytest.fixture(scope="module")
def rand300():
    return X.random_batch(300)


def up(a, view):
    import torch
    return torch.from_numpy(a.view(view).copy()).cuda()


def run(ex, cases, rna=False, device=False, cigar_lead=0):
    a = X.layout(cases, cigar_lead)
    ops = (up(a["op_n"], np.int32), up(a["op_off"], np.int64), up(a["query_start"], np.int32), up(a["status"], np.int32))
    cg = (up(a["cigar"], np.int32), up(a["cigar_off"], np.int64), up(a["pos"], np.int32)) if device else (a["cigar"], a["cigar_off"], a["pos"])
    return ex.project(ops, *cg, rna=rna)


def same(res, cases, rna=False):
    want = X.expected(cases, rna)
    got = res.to_host()
    for key in ("status", "op_off", "op_n", "op_t", "query_start", "query_end", "target_start", "target_end", "ref_len", "n_match"):
        assert np.array_equal(got[key], want[key]), (key, [c.label for c, a, b in zip(cases, got[key], want[key]) if key not in ("op_n", "op_t", "op_off") and a != b][:5])
    assert np.array_equal(res.status, want["status"]) and np.array_equal(res.ref_len_host, want["ref_len"])
    assert np.array_equal(res.n_match_host, want["n_match"]) and np.array_equal(res.query_end_host, want["query_end"])
    assert res.n_ops == int(want["op_off"][-1]) == got["op_t"].size
    refused = np.flatnonzero(want["status"] != 0)
    assert res.n_refused == refused.size and res.first_refused == (int(refused[0]) if refused.size else -1)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("rna", [False, True])
def test_every_edge_case_in_one_batch(ex, edge, rna, device):
    same(run(ex, edge, rna, device, cigar_lead=3 if device else 0), edge, rna)   # refused reads lie between accepted ones


@pytest.mark.parametrize("rna", [False, True])
def test_every_edge_case_alone(ex, edge, rna):
    for c in edge:
        same(run(ex, [c], rna), [c], rna)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("rna", [False, True])
def test_batches_of_0_1_and_300_reads(ex, rand300, rna, device):
    res = run(ex, [], rna, device)
    assert res.n_reads == 0 and res.n_ops == 0 and res.first_refused == -1 and res.op_off.cpu().tolist() == [0]
    same(run(ex, rand300[:1], rna, device), rand300[:1], rna)
    same(run(ex, rand300, rna, device), rand300, rna)


def test_one_shot_and_the_issues_example():
    from poregen_amd.engine import project_ops
    o = np.arange(10, 20, dtype=np.uint32)
    c = X.Case("example", o, X.R.words_of("2S3M1I2M2D2M"))
    a = X.layout([c])
    for rna, ops, qs, t in ((False, [12, 13, 14, 15, 16, 17, 2, 18, 19], 121, (1000, 1009)), (True, [10, 11, 2, 12, 13, 14, 15, 16, 17], 100, (1009, 1000))):
        out = project_ops(a["op_n"], a["op_off"], a["query_start"], a["status"], a["cigar"], a["cigar_off"], a["pos"], rna=rna)
        assert out["op_n"].tolist() == ops and out["query_start"].tolist() == [qs] and (int(out["target_start"][0]), int(out["target_end"][0])) == t
        assert out["n_match"].tolist() == [7] and out["ref_len"].tolist() == [9] and out["n_ops"] == 9 and out["n_refused"] == 0
        assert out["op_t"].tolist() == ([0, 0, 0, 1, 0, 0, 2, 0, 0] if not rna else [0, 0, 2, 0, 0, 1, 0, 0, 0])


@pytest.mark.parametrize("rna", [False, True])
def test_expansion_projected_in_place(ex, rna):
    """pg_mvops_expand's result, read where it lies: accepted and refused tables, each with a CIGAR over its bases."""
    rng = np.random.default_rng(11)
    reads = [r for _, r in M.edge_reads(ex.piece)][:40]
    a = M.layout(reads)
    flags = MR.RNA if rna else 0
    mo = ex.expand(a["mv"], a["mv_off"], a["stride"], a["ns"], a["ts"], a["l_seq"], a["flag"], a["seq_bytes"], a["byte_off"], rna=rna)
    refs = [r.ref(flags) for r in reads]
    cases = [X.Case(f"mv{i}", f.ops, X.edit_words(rng, len(r.codes)) if len(r.codes) else X.R.words_of("2D"), qs=f.query_start if f.status == 0 else 0, status=f.status, pos=77 + i)
             for i, (r, f) in enumerate(zip(reads, refs))]
    assert any(c.status for c in cases) and any(c.status == 0 and len(c.o) > 1000 for c in cases)
    lay = X.layout(cases)
    res = ex.project(mo, lay["cigar"], lay["cigar_off"], lay["pos"], rna=rna)
    want, got = X.expected(cases, rna), res.to_host()
    ok = want["status"] == 0
    for key in ("status", "op_off", "op_n", "op_t", "target_start", "target_end", "ref_len", "n_match"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["query_start"][ok], want["query_start"][ok]) and np.array_equal(got["query_end"][ok], want["query_end"][ok])
    assert np.array_equal(mo.to_host()["op_n"], M.expected(reads, flags)["op_n"])          # the expansion's result is left as it is


def test_refused_arguments(ex, edge):
    import torch
    from poregen_amd import _abi
    from poregen_amd.engine import PgError
    cases = [c for c in edge if c.status == 0][:6]
    a = X.layout(cases)
    ops = (up(a["op_n"], np.int32), up(a["op_off"], np.int64), up(a["query_start"], np.int32), up(a["status"], np.int32))
    down = a["cigar_off"].copy(); down[2], down[3] = down[3], down[2]
    beyond = a["cigar_off"].copy(); beyond[-1] += 1
    for off in (down, beyond):
        for dev in (False, True):
            with pytest.raises(PgError) as ei:
                ex.project(ops, up(a["cigar"], np.int32) if dev else a["cigar"], up(off, np.int64) if dev else off, up(a["pos"], np.int32) if dev else a["pos"])
            assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "cigar_off" in str(ei.value)
    past = a["op_off"].copy(); past[-1] += 1
    bad_ops = (ops[0], up(past, np.int64), ops[2], ops[3])
    with pytest.raises(PgError) as ei:
        ex.project(bad_ops, a["cigar"], a["cigar_off"], a["pos"])
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        ex.project((ops[0].cpu(), ops[1], ops[2], ops[3]), a["cigar"], a["cigar_off"], a["pos"])
    same(run(ex, cases), cases)                              # the handle stays usable
