"""What the pooled entry points of the façade share, without a GPU: the one description of a call's pools (demux._pool_setup), the host
layout of a pooled call (pools.pooled_layout, against the row_ptr of tests/pools_restatement.py) and the two managers of a private
context's lifetime (demux._generator_context, demux._handed_over_context) on a recording stand-in."""
from types import SimpleNamespace

import numpy as np
import pytest

from demuxalot_amd import demux
from demuxalot_amd.pools import pooled_layout
from tests import pools_restatement as restated


def _inputs(n_donors, barcodes=('b0', 'b1', 'b2', 'b3')):
    names = [chr(ord('A') + g) for g in range(n_donors)] if n_donors <= 26 else [f'D{g:02d}' for g in range(n_donors)]
    return (SimpleNamespace(genotype_names=names, n_genotypes=n_donors),
            SimpleNamespace(ordered_barcodes=list(barcodes), n_barcodes=len(barcodes)))


def _bonus(n_donors, doublet_prior):
    """The reference's pair bonus (demux.py:164-169) for a genotype list of n_donors > 1, as float32."""
    slots = n_donors * (n_donors - 1) / 2
    return np.float32(np.log(n_donors * doublet_prior) - np.log(slots * (1 - doublet_prior)))


# ---- the resolver --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('doublet_prior', [0.0, 0.35])
def test_setup_of_three_donors_in_two_pools(doublet_prior):
    genotypes, handler = _inputs(3)
    barcode2pool = {'b0': 'small', 'b1': 'big', 'b2': 'big', 'b3': 'small'}
    pool2donors = {'small': ['C', 'A'], 'big': ['B', 'C', 'A']}  # (any order: sorted into genotype order)
    setup = demux._pool_setup(genotypes, handler, doublet_prior, barcode2pool, pool2donors, 'an_entry')
    assert setup.pooled is True
    assert setup.pool_names == ['small', 'big']
    assert [list(c) for c in setup.pool_columns] == [[0, 2], [0, 1, 2]]
    assert setup.pool_of_barcode.dtype == np.int32 and setup.pool_of_barcode.tolist() == [0, 1, 1, 0]
    assert setup.pair_penalty.dtype == np.float32 and setup.pair_penalty.shape == (2,)
    if doublet_prior == 0:
        assert setup.option_names == [['A', 'C'], ['A', 'B', 'C']]
        assert setup.pair_penalty.tolist() == [0.0, 0.0]
    else:
        assert setup.option_names == [['A', 'C', 'A+C'], ['A', 'B', 'C', 'A+B', 'A+C', 'B+C']]
        assert setup.pair_penalty[0] == _bonus(2, 0.35) and setup.pair_penalty[1] == _bonus(3, 0.35)
        assert abs(float(setup.pair_penalty[0]) - 0.0741080) < 1e-6 and abs(float(setup.pair_penalty[1]) + 0.6190392) < 1e-6


def test_setup_of_a_one_donor_pool_and_a_barcode_in_no_pool():
    genotypes, handler = _inputs(3)
    barcode2pool = {'b0': 'one', 'b1': None, 'b2': 'two', 'b3': 'one'}
    setup = demux._pool_setup(genotypes, handler, 0.35, barcode2pool, {'one': ['B'], 'two': ['A', 'C']}, None)
    assert setup.pooled is True  # (who=None: an entry that takes pools only)
    assert setup.pool_of_barcode.tolist() == [0, -1, 1, 0]
    assert setup.option_names == [['B'], ['A', 'C', 'A+C']]
    assert setup.pair_penalty[0] == 0.0 and not np.signbit(setup.pair_penalty[0])  # exactly 0.0: one donor has no pair
    assert setup.pair_penalty[1] == _bonus(2, 0.35)


def test_setup_without_pools_is_one_pool_of_everybody():
    genotypes, handler = _inputs(3)
    setup = demux._pool_setup(genotypes, handler, 0.35, None, None, 'an_entry')
    assert setup.pooled is False
    assert setup.pool_names == ['all']
    assert [list(c) for c in setup.pool_columns] == [[0, 1, 2]]
    assert setup.pool_of_barcode.dtype == np.int32 and setup.pool_of_barcode.tolist() == [0, 0, 0, 0]
    assert setup.option_names == [['A', 'B', 'C', 'A+B', 'A+C', 'B+C']]
    assert setup.pair_penalty.dtype == np.float32 and setup.pair_penalty.tolist() == [_bonus(3, 0.35)]


def test_setup_without_pools_refuses_more_options_than_one_pool_holds():
    genotypes, handler = _inputs(46)
    with pytest.raises(ValueError, match=r'^the_entry_that_asked: 46 donors make 1081 options, more than the 1024 one pool can hold'):
        demux._pool_setup(genotypes, handler, 0.35, None, None, 'the_entry_that_asked')


def test_setup_without_pools_accepts_45_singlets():
    genotypes, handler = _inputs(45)
    setup = demux._pool_setup(genotypes, handler, 0.0, None, None, 'an_entry')
    assert setup.pooled is False and [list(c) for c in setup.pool_columns] == [list(range(45))]
    assert setup.option_names == [genotypes.genotype_names] and setup.pair_penalty.tolist() == [0.0]


# ---- the layout ----------------------------------------------------------------------------------------------------------------
_PROBLEM = restated.fixture_problem('f3_small_2.npz')  # (v, cb, e, prob, B): 5 donors


def _restated_row_ptr(pools, pool_of_barcode, doublet_prior):
    v, cb, e, prob, B = _PROBLEM
    n = len(pool_of_barcode)
    assert n <= B
    keep = cb < n  # the first n barcodes of the problem
    return restated.Restatement(v[keep], cb[keep], e[keep], prob, n, doublet_prior)(pools, pool_of_barcode)['row_ptr']


@pytest.mark.parametrize('with_doublets', [False, True])
@pytest.mark.parametrize('pools, pool_of_barcode', [
    ([], [-1, -1, -1]),                      # an empty pool list
    ([[0, 2], [1, 2, 4]], []),               # B = 0
    ([[0, 2], [1, 2, 4], [3]], [-1] * 6),    # all barcodes in no pool
    ([[0, 2], [1, 2, 4], [3]], [0, 3, 1, 2, -1, 1, 3]),  # an id equal to len(pools): a row of length 0, left for the library to refuse
], ids=['no-pools', 'no-barcodes', 'all-unpooled', 'id-past-the-pools'])
def test_layout_follows_the_restatement(pools, pool_of_barcode, with_doublets):
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
    pool_start, donors, row_ptr = pooled_layout(pools, pool_of_barcode, with_doublets)
    assert pool_start.dtype == np.int64 and pool_start.tolist() == [0] + list(np.cumsum([len(d) for d in pools]))
    assert donors.dtype == np.int32 and donors.flags.c_contiguous and donors.tolist() == [g for d in pools for g in d]
    want = _restated_row_ptr(pools, pool_of_barcode, 0.35 if with_doublets else 0.0)
    assert row_ptr.dtype == np.int64 and row_ptr.shape == (len(pool_of_barcode) + 1,)
    assert np.array_equal(row_ptr, want)


def test_layout_row_lengths_written_out():
    pools, pool_of = [[0, 2], [1, 2, 4], [3]], np.array([0, 3, 1, 2, -1, 1], np.int32)
    assert pooled_layout(pools, pool_of, True)[2].tolist() == [0, 3, 3, 9, 10, 10, 16]
    assert pooled_layout(pools, pool_of, False)[2].tolist() == [0, 2, 2, 5, 6, 6, 9]


# ---- the lifetime of a private context -----------------------------------------------------------------------------------------
class _RecordingContext:
    def __init__(self):
        self.closed = 0

    def close(self):
        self.closed += 1


@pytest.fixture
def private_contexts(monkeypatch):
    """acquire / release of the device layer replaced by a record: [(event, context, failed)]."""
    record = []

    def acquire(device=None):
        ctx = _RecordingContext()
        record.append(('acquire', ctx, None))
        return ctx

    monkeypatch.setattr(demux, 'acquire_private_context', acquire)
    monkeypatch.setattr(demux, 'release_private_context', lambda ctx, failed=False: record.append(('release', ctx, failed)))
    return record


def _staged(fail_after_first=False):
    with demux._generator_context() as ctx:
        yield ctx
        if fail_after_first:
            raise RuntimeError('the body failed')
        yield ctx


def test_generator_context_is_lazy_and_releases_once_at_the_end(private_contexts):
    generator = _staged()
    assert private_contexts == []  # nothing before the first next
    contexts = list(generator)
    assert len(contexts) == 2 and contexts[0] is contexts[1]
    assert [(event, failed) for event, _ctx, failed in private_contexts] == [('acquire', None), ('release', False)]
    assert private_contexts[1][1] is contexts[0] and contexts[0].closed == 0


def test_generator_context_releases_once_when_the_consumer_stops_early(private_contexts):
    generator = _staged()
    ctx = next(generator)
    generator.close()
    assert [(event, failed) for event, _ctx, failed in private_contexts] == [('acquire', None), ('release', False)]
    assert private_contexts[1][1] is ctx and ctx.closed == 0


def test_generator_context_releases_as_failed_when_the_body_raises(private_contexts):
    generator = _staged(fail_after_first=True)
    ctx = next(generator)
    with pytest.raises(RuntimeError, match='the body failed'):
        next(generator)
    assert [(event, failed) for event, _ctx, failed in private_contexts] == [('acquire', None), ('release', True)]
    assert private_contexts[1][1] is ctx


def test_handed_over_context_closes_on_failure_and_stays_open_on_success(private_contexts):
    with demux._handed_over_context() as kept:
        pass
    assert kept.closed == 0
    with pytest.raises(KeyError):
        with demux._handed_over_context() as lost:
            raise KeyError('the call failed')
    assert lost.closed == 1 and kept.closed == 0
    assert [event for event, _ctx, _failed in private_contexts] == ['acquire', 'acquire']  # neither goes back to the pool: closed, or the result's
