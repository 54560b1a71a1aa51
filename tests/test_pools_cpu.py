"""Host side of the pooled posteriors (demuxalot_amd/pools.py) and the proof of their checker (tests/pools_restatement.py) against the
reference's own captured outputs: runs without a GPU."""
import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pools_restatement as restated


@pytest.mark.parametrize('name', ['f2_synthetic_g4.npz', 'f3_small_2.npz', 'f1_synthetic_default.npz'])
def test_restatement_with_one_all_donor_pool_is_the_reference(name):
    fx = fio.load(name)
    G, B = len(fx['genotype_names']), len(fx['barcodes'])
    for i in range(int(fx['n_predict'])):
        dp, clip = float(fx[f'predict{i}_dp']), float(fx[f'predict{i}_clip'])
        v, cb, e, prob, n = restated.fixture_problem(name, clip)
        assert n == B
        want = restated.Restatement(v, cb, e, prob, B, dp)([list(range(G))], np.zeros(B, np.int32))
        K = fx[f'predict{i}_logits'].shape[1]
        assert np.array_equal(want['row_ptr'], np.arange(B + 1) * K)
        fio.assert_bitwise(want['logits'].reshape(B, K), fx[f'predict{i}_logits'], f'{name} predict {i}: logits')
        fio.assert_bitwise(want['probs'].reshape(B, K), fx[f'predict{i}_probs'], f'{name} predict {i}: probs')
        reference = fx[f'predict{i}_probs']
        assert np.array_equal(want['best_option'], reference.argmax(axis=1))
        fio.assert_bitwise(want['best_prob'], reference.max(axis=1), 'best_prob')
        if dp == 0:
            assert not want['doublet_mass'].any()
        else:
            assert np.allclose(want['doublet_mass'], reference[:, G:].astype(np.float64).sum(axis=1), rtol=1e-12, atol=0)


def test_restatement_cuts_rows_and_skips_barcodes_of_no_pool():
    v, cb, e, prob, B = restated.fixture_problem('f3_small_2.npz')
    r = restated.Restatement(v, cb, e, prob, B, 0.35)
    pools = [[0, 2], [1, 2, 4], [3]]
    pool_of = np.array([b % 4 - 1 for b in range(B)], np.int32)  # -1, 0, 1, 2, ...
    want = r(pools, pool_of)
    assert list(np.diff(want['row_ptr'])[:4]) == [0, 3, 6, 1]
    for b in range(B):
        row = want['probs'][want['row_ptr'][b]:want['row_ptr'][b + 1]]
        if pool_of[b] < 0:
            assert want['best_option'][b] == -1 and np.isnan(want['best_prob'][b]) and np.isnan(want['doublet_mass'][b])
            continue
        fio.assert_bitwise(row, r.pool_rows(pools[pool_of[b]])[1][b], f'row {b}')
        assert want['best_option'][b] == row.argmax() and want['best_prob'][b] == row.max()
        mass = 0.0
        for x in row[len(pools[pool_of[b]]):]:
            mass += float(x)
        assert want['doublet_mass'][b] == mass
    single = want['probs'][want['row_ptr'][3]:want['row_ptr'][4]]
    assert list(single) == [1.0] and want['doublet_mass'][3] == 0.0  # one donor: one option, no pairs
    assert list(r.pair_penalty(pools)[2:]) == [0.0] and r.pair_penalty(pools)[0] != 0


NAMES = ['d0', 'd1', 'd2', 'd3']
BARCODES = ['b0', 'b1', 'b2']


def test_resolve_pools_sorts_donors_into_genotype_order():
    from demuxalot_amd.pools import resolve_pools
    names, columns, pool_of = resolve_pools(NAMES, BARCODES, {'b0': 'B', 'b1': None, 'b2': 'A'}, {'A': ['d1', 'd0'], 'B': ('d3', 'd1', 'd2')})
    assert names == ['A', 'B'] and columns == [[0, 1], [1, 2, 3]]
    assert pool_of.dtype == np.int32 and list(pool_of) == [1, -1, 0]


@pytest.mark.parametrize('barcode2pool, pool2donors, message', [
    ({'b0': 'A', 'b1': 'A', 'b2': 'A'}, {'A': ['d0', 'd0']}, 'more than once'),
    ({'b0': 'A', 'b1': 'A', 'b2': 'A'}, {'A': ['d0', 'dX']}, 'unknown donor'),
    ({'b0': 'A', 'b1': 'A', 'b2': 'A'}, {'A': []}, 'no donors'),
    ({'b0': 'A', 'b1': 'A'}, {'A': ['d0']}, 'missing from barcode2pool'),
    ({'b0': 'A', 'b1': 'A', 'b2': 'C'}, {'A': ['d0']}, 'unknown pool'),
])
def test_resolve_pools_refuses(barcode2pool, pool2donors, message):
    from demuxalot_amd.pools import resolve_pools
    with pytest.raises(ValueError, match=message):
        resolve_pools(NAMES, BARCODES, barcode2pool, pool2donors)


def test_predict_posteriors_in_pools_validates_before_it_touches_a_device():
    """The name checks come first: they raise without a GPU (and without a library call)."""
    from demuxalot_amd import BarcodeHandler, Demultiplexer, ProbabilisticGenotypes
    genotypes = ProbabilisticGenotypes(NAMES)
    handler = BarcodeHandler(BARCODES)
    with pytest.raises(ValueError, match='unknown donor'):
        Demultiplexer.predict_posteriors_in_pools({}, genotypes, handler, {b: 'A' for b in BARCODES}, {'A': ['d0', 'nobody']})
    with pytest.raises(ValueError, match='missing from barcode2pool'):
        Demultiplexer.predict_posteriors_in_pools({}, genotypes, handler, {'b0': 'A'}, {'A': ['d0']})


def hand_made():
    from demuxalot_amd import PooledPosteriors
    from demuxalot_amd.demux import _option_names
    columns = [_option_names(['d0', 'd1'], 0.35), _option_names(['d1', 'd2', 'd3'], 0.35)]
    assert columns == [['d0', 'd1', 'd0+d1'], ['d1', 'd2', 'd3', 'd1+d2', 'd1+d3', 'd2+d3']]
    pool_of = np.array([1, -1, 0, 1], np.int32)
    row_ptr = np.array([0, 6, 6, 9, 15], np.int64)
    probs = np.array([.1, .1, .1, .5, .1, .1, .05, .95, 0., 0., 0., .25, .25, .25, .25], np.float32)
    logits = np.log(probs.clip(1e-30)).astype(np.float32)
    best_option = np.array([3, -1, 1, 2], np.int32)
    best_prob = np.array([.5, np.nan, .95, .25], np.float32)
    mass = np.array([.7, np.nan, 0., .75], np.float64)
    return PooledPosteriors(['w', 'x', 'y', 'z'], ['A', 'B'], columns, pool_of, row_ptr, logits, probs, best_option, best_prob, mass), logits, probs


def test_pooled_posteriors_from_hand_made_arrays():
    pooled, logits, probs = hand_made()
    assert pooled.pools == ['A', 'B']
    assert pooled.barcodes_of('A') == ['y'] and pooled.barcodes_of('B') == ['w', 'z']
    assert pooled.columns_of('A') == ['d0', 'd1', 'd0+d1']
    logits_df, probs_df = pooled.to_dataframes('B')
    assert list(probs_df.index) == ['w', 'z'] and probs_df.index.name == 'BARCODE' and logits_df.index.name == 'BARCODE'
    assert list(probs_df.columns) == ['d1', 'd2', 'd3', 'd1+d2', 'd1+d3', 'd2+d3'] and list(logits_df.columns) == list(probs_df.columns)
    assert probs_df.values.dtype == np.float32 and logits_df.values.dtype == np.float32
    fio.assert_bitwise(probs_df.values, np.stack([probs[0:6], probs[9:15]]), 'pool B probs')
    fio.assert_bitwise(logits_df.values, np.stack([logits[0:6], logits[9:15]]), 'pool B logits')
    fio.assert_bitwise(pooled.to_dataframes('A')[1].values, probs[6:9][None, :], 'pool A probs')
    best = pooled.best()
    assert list(best.columns) == ['pool', 'option', 'probability'] and list(best.index) == ['w', 'x', 'y', 'z']
    assert list(best['pool']) == ['B', None, 'A', 'B'] and list(best['option']) == ['d1+d2', None, 'd1', 'd3']
    assert np.isnan(best['probability'].values[1]) and best['probability'].values.dtype == np.float32
    assigned = pooled.assignments(0.9)
    assert list(assigned.index) == ['y'] and list(assigned) == ['d1']
    assert list(pooled.assignments(0.2).index) == ['w', 'y', 'z']
    assert list(pooled.assignments(0.5).index) == ['y']  # strictly above, as Series.gt
    dp = pooled.doublet_probability()
    assert dp.dtype == np.float64 and list(dp.index) == ['w', 'x', 'y', 'z'] and dp['w'] == .7 and np.isnan(dp['x'])
    with pytest.raises(KeyError):
        pooled.to_dataframes('C')


def test_pooled_posteriors_checks_its_row_pointer():
    from demuxalot_amd import PooledPosteriors
    with pytest.raises(AssertionError):
        PooledPosteriors(['w'], ['A'], [['d0', 'd1']], [0], [0, 3], np.zeros(3), np.zeros(3), [0], [1.0], [0.0])
