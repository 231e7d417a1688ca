"""SignalMeans.submit_svb on the MI355X: the means, the fallback count and the dataset summary of svb-zd blocks decoded on the device
are, bit for bit, those of submit() on the samples tests/sigdec_ref.py decodes the same blocks to."""
import numpy as np
import pytest
import torch

import pamean_ref as R
import sigdec_cases as K
import sigdec_ref as S
from poregen_amd import _abi
from poregen_amd.engine import PgError, SignalMeans, read_means, read_means_svb
from test_gpu_pamean import batch, records

pytestmark = pytest.mark.gpu


def svb_batch(recs):
    """(blocks, block_off, digitisation, offset, range) of records, and the samples the reference decodes the blocks to"""
    blks = [S.encode(r[1]) for r in recs]
    for b, r in zip(blks, recs):
        assert np.array_equal(S.decode(b), r[1])
    blocks, boff = K.pack(blks)
    return (blocks, boff, np.array([r[2] for r in recs]), np.array([r[3] for r in recs]), np.array([r[4] for r in recs]))


def same(a, b):
    assert a.means.tobytes() == b.means.tobytes()
    assert (a.n_fallback, a.n_samples) == (b.n_fallback, b.n_samples)
    assert np.float64(a.mean).tobytes() == np.float64(b.mean).tobytes() and np.float64(a.sstdev).tobytes() == np.float64(b.sstdev).tobytes()


@pytest.fixture(scope="module")
def recs():
    return records(seed=3)


def test_submit_svb_is_submit_on_the_decoded_samples(recs):
    want = read_means(*batch(recs))
    sb = svb_batch(recs)
    sm = SignalMeans()
    assert sm.svb_samples == 0
    sm.submit_svb(*sb)
    assert sm.svb_samples == want.n_samples == sum(len(r[1]) for r in recs)
    got = sm.finish()
    same(got, want)
    sm.submit(*batch(recs[:7]))                       # plain submit decodes nothing on the device
    sm.finish()
    assert sm.svb_samples == want.n_samples
    sm.submit_svb(torch.from_numpy(sb[0]).cuda(), *sb[1:])     # device blocks
    same(sm.finish(), want)
    assert sm.svb_samples == 2 * want.n_samples
    sm.close()
    plain = SignalMeans()
    plain.submit(*batch(recs))
    plain.finish()
    assert plain.svb_samples == 0
    plain.close()


def test_batches_of_blocks_and_of_samples_mix(recs):
    want = read_means(*batch(recs))
    sm = SignalMeans()
    for k, a in enumerate(range(0, len(recs), 9)):
        part = recs[a:a + 9]
        if k % 2:
            sm.submit(*batch(part))
        else:
            sm.submit_svb(*svb_batch(part))
    same(sm.finish(), want)
    sm.close()


def test_reads_that_fall_back_are_copied_from_the_decoded_samples():
    recs = R.boundary_reads(200_000, 6, seed=29)
    want = read_means(*batch(recs))
    got = read_means_svb(*svb_batch(recs))
    assert want.n_fallback >= len(recs)
    same(got, want)
    assert [R.fmt_f(m) for m in got.means] == [R.fmt_f(R.seq_mean(*x[1:])) for x in recs]


def test_a_corrupt_block_fails_the_batch_and_the_handle_goes_on(recs):
    part = recs[:12]
    blocks, boff, dig, off, rng = svb_batch(part)
    zz, nb = K.case("alternating", 2 * K.V_PIECE + 1, np.random.default_rng(4))
    short = S.encode_values(zz, nb)[:-2]              # passes the host's checks; its byte lengths run past its data
    assert S.check(len(short), zz.size) == 0 and S.decode(short) is None
    blks = [S.encode(r[1]) for r in part]
    blks.insert(5, short)
    b2, o2 = K.pack(blks)
    ins = lambda a: np.insert(a, 5, a[0])             # noqa: E731
    sm = SignalMeans()
    with pytest.raises(PgError) as ei:
        sm.submit_svb(b2, o2, ins(dig), ins(off), ins(rng))
    assert ei.value.status == _abi.PG_ERR_INPUT and "read 5" in ei.value.text and "corrupt streamvbyte block" in ei.value.text
    assert sm.svb_samples == 0
    sm.submit_svb(blocks, boff, dig, off, rng)
    same(sm.finish(), read_means(*batch(part)))
    sm.close()
