"""tests/pooled_helpers.py judges the GPU tests of every pooled entry, so its comparisons are shown to bite here, without a GPU: one
changed bit, another type, the sign of a zero.  The designed problems those tests run on were tuned to sit on kernel edges; a SHA-256
over the bytes of every array they hold is pinned, so that an edit of a generator cannot move them silently."""
import hashlib

import numpy as np
import pytest

from tests import pair_shares_restatement
from tests import pooled_helpers as helpers
from tests import test_gpu_ambient_grid, test_gpu_ambient_marginal, test_gpu_ambient_scoring


def one_ulp_up(array, at=0):
    out = np.array(array, copy=True)
    out.reshape(-1)[at] = np.nextafter(out.reshape(-1)[at], out.dtype.type(np.inf))
    return out


# ---- same_bytes -------------------------------------------------------------------------------------------------------------------
def test_same_bytes_sees_a_bit_a_type_and_the_sign_of_a_zero():
    want = dict(a=np.array([0.0, 1.5, -2.0], np.float32), n=np.arange(4, dtype=np.int32))
    helpers.same_bytes(dict(a=want['a'].copy(), n=want['n'].copy()), want, ('a', 'n'), 'equal')
    flipped = want['a'].copy()
    flipped.view(np.uint32)[1] ^= 1
    for key, other in (('a', flipped), ('n', want['n'].astype(np.int64)), ('a', want['a'].astype(np.float64)),
                       ('a', np.array([-0.0, 1.5, -2.0], np.float32))):
        assert np.array_equal(other, want[key]) or key == 'a' and other is flipped
        with pytest.raises(AssertionError, match=f'what: {key}'):
            helpers.same_bytes({**want, key: other}, want, ('a', 'n'), 'what')
    helpers.same_bytes({**want, 'a': flipped}, want, ('n',), 'a key that is not asked for is not compared')


# ---- assert_iteration -------------------------------------------------------------------------------------------------------------
class Context:
    """What assert_iteration asks of a context, and what a test asks beside it."""

    def __init__(self, dense):
        self.dense = dense

    def get_probs(self):
        return self.dense

    def get_learnt_betas(self):
        raise AssertionError('assert_iteration does not judge the betas')

    def timings(self):
        raise AssertionError('assert_iteration launches and times nothing')


def iteration():
    """(got, want): a record of two barcodes, the second in no pool, as a pooled E-step and its restatement hold it."""
    nan = np.nan
    rows = dict(row_ptr=np.array([0, 3, 3], np.int64), logits=np.array([-1.0, -2.5, -0.25], np.float32), probs=np.array([0.25, 0.125, 0.625], np.float32),
                best_option=np.array([2, -1], np.int32), best_prob=np.array([0.625, nan], np.float32), doublet_mass=np.array([0.625, nan], np.float64))
    want = dict(rows, dense=np.array([[0.25, 0.125], [0.0, 0.0]], np.float32), addition=np.array([[1.0, 2.0], [0.5, 0.0]], np.float32),
                ambient=np.array([0.5, 0.25], np.float32))
    got = {key: value.copy() for key, value in rows.items()}
    return got, want


def test_assert_iteration_sees_one_ulp_in_the_dense_matrix_the_addition_and_the_soup():
    got, want = iteration()
    ctx = Context(want['dense'].copy())
    helpers.assert_iteration(ctx, got, want, 'equal')
    helpers.assert_iteration(ctx, got, want, 'equal', want['addition'].copy())
    helpers.assert_iteration(ctx, dict(got, ambient=want['ambient'].copy()), want, 'equal, with a soup profile', want['addition'].copy())
    with pytest.raises(AssertionError, match='get_probs'):
        helpers.assert_iteration(Context(one_ulp_up(want['dense'], 1)), got, want, 'what')
    with pytest.raises(AssertionError, match='addition'):
        helpers.assert_iteration(ctx, got, want, 'what', one_ulp_up(want['addition'], 2))
    with pytest.raises(AssertionError, match='soup'):
        helpers.assert_iteration(ctx, dict(got, ambient=one_ulp_up(want['ambient'], 1)), want, 'what')
    with pytest.raises(AssertionError, match='probs'):
        helpers.assert_iteration(ctx, dict(got, probs=one_ulp_up(got['probs'], 2)), want, 'what')
    seen = []
    helpers.assert_iteration(ctx, got, want, 'another judge of the rows', same=lambda *args: seen.append(args))
    assert len(seen) == 1 and seen[0][0] is got and seen[0][1] is want


# ---- pool_refusal_cases -----------------------------------------------------------------------------------------------------------
def test_pool_refusal_cases_change_what_they_say():
    B = 7
    pool_of = np.where(np.arange(B) % 5 == 4, -1, np.arange(B) % 2).astype(np.int32)
    good = dict(with_doublets=1, pool_start=[0, 2, 5], donors=[0, 1, 1, 2, 4], penalty=np.array([0.25, -0.5], np.float32), pool_of=pool_of,
                row_ptr=np.array([0, 3, 9, 12, 18, 18, 24, 27], np.int64), alpha=np.zeros(B, np.float32))
    before = {key: np.array(value, copy=True) for key, value in good.items()}
    cases = helpers.pool_refusal_cases(good, pool_of)
    assert [message for _change, _code, message in cases] == ['pool_start[0]', 'empty', 'ascending', 'outside', 'pool_of_barcode', 'row_ptr',
                                                              'with_doublets', 'n_pools']
    assert all(code == helpers.DMX_ERR_INVALID for _change, code, _message in cases)
    changed = [sorted(change) for change, _code, _message in cases]
    assert changed == [['pool_start'], ['penalty', 'pool_start'], ['donors'], ['donors'], ['pool_of'], ['row_ptr'], ['with_doublets'], ['n_pools']]

    def differs(key, value):
        a, b = np.asarray(value), np.asarray(good[key])
        return None if a.shape != b.shape else np.flatnonzero(a != b).tolist()

    by_message = {message: change for change, _code, message in cases}
    assert differs('pool_start', by_message['pool_start[0]']['pool_start']) == [0]
    assert by_message['empty']['pool_start'] == [0, 2, 2, 5] and len(by_message['empty']['penalty']) == 3, 'three pools, the second empty'
    assert differs('donors', by_message['ascending']['donors']) == [2, 3] and by_message['ascending']['donors'][2] > by_message['ascending']['donors'][3]
    assert differs('donors', by_message['outside']['donors']) == [4] and by_message['outside']['donors'][4] == 5, 'G = 5: the first column outside'
    assert differs('pool_of', by_message['pool_of_barcode']['pool_of']) == [1] and by_message['pool_of_barcode']['pool_of'][1] == 2
    assert differs('row_ptr', by_message['row_ptr']['row_ptr']) == list(range(1, B + 1))
    assert by_message['with_doublets']['with_doublets'] == 2 and by_message['n_pools']['n_pools'] == -1 and 'n_pools' not in good
    for key, value in good.items():
        assert np.array_equal(np.asarray(value), before[key]), f'{key}: the good call itself is left alone'
    with pytest.raises(AssertionError):
        helpers.pool_refusal_cases(dict(good, donors=[0, 1, 2, 3, 4]), pool_of)


# ---- the designed problems' bytes -------------------------------------------------------------------------------------------------
def digest(arrays):
    """SHA-256 over type, shape and bytes of every array, in their order."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# (v, cb, e, prob, v2snp, soup, lengths) of the three GPU modules' designed problems; the scoring and the grid module share one problem
DESIGNED_DIGESTS = {
    test_gpu_ambient_scoring: 'fba222f3483751e135483084a8dd81998b6793788d21ae3ebdd2079d93744286',
    test_gpu_ambient_grid: 'fba222f3483751e135483084a8dd81998b6793788d21ae3ebdd2079d93744286',
    test_gpu_ambient_marginal: '2492deaf2f45aeaef79609853c863825977849dabc090750b1feaefef0a80ad7',
}
PAIR_SHARES_DIGEST = 'b8959deb0ecaf5e4e58244f99f41bde142fef29e22ce385c9e0b880142b2654d'  # (v, cb, e, prob, v2snp, lengths): it has no soup
GRID_DIGESTS = {  # designed_grid(n, seed_base) for the lengths the GPU tests use: the ambient grids (100), the shares (300)
    100: {1: '42e977b96a41a1053d01f2030224b1ae18ca41fd75741e498d2c73426a2cf8fb', 2: '21c6068fb2501e0447e4280063dd4431454cc4e38c52fab9d1eb80585f2d6958',
          3: '26e9e9b37da71015cf53635184b027c665837b2d6efa6cacf2a5685419405ab9', 4: '5f76ae38582991148848d34a95f68e6603549e93065578b82532ef456063ddc9',
          5: '08b41924ed7d6f9c24bdedf26a294b636f1f2c0512c62dcecd2b328730c53ac7', 8: 'fc82a3c83bc918c47bf8d9184835f967c8818ad7ac8f5bce90d0e8d319e075bc',
          9: 'e0563c37841ab000d95cb8a248e3c0ecde2006387fbf285eb48805e7c3ad4725', 63: '8fe6d9a1fb2b59e9002880e2a2568863e28d9158a5f84d237d131c82bc6c38e8',
          64: '7d016b4bd29b23b991f9d6ae9ea3f58136a4ef56c62d47ea01143d08b54f4bdf'},
    300: {1: '9bad7dc36cf52dc8351c456405e5f4f5f77b94fc6a2d7c5c28f690aa5e2ef2b0', 2: '21c6068fb2501e0447e4280063dd4431454cc4e38c52fab9d1eb80585f2d6958',
          3: '26e9e9b37da71015cf53635184b027c665837b2d6efa6cacf2a5685419405ab9', 4: '5732604a79ed2cd9cf557c3220639233db9f4c8a77be7bf71275abc948871d88',
          5: '56e1a4d43b73e87921b1b3573527e442343d933a981baa65cd7c34cc0701de09', 8: 'b48d71bada5ab6fdb7c09e1615c4b5cc4225d0c45c66c2f18821a372a1f964e9',
          9: '90c480618c4a3c59d13d6b43526810ff620d04f0a8851796c1dd74b3003b1bd0', 64: '5f9318e3cf6cec95bbefda1de5980ddffe1192e0dbaa6bd1227053a5e55c4f5d'},
}


def test_the_designed_problems_hold_the_pinned_bytes():
    for module, want in DESIGNED_DIGESTS.items():
        arrays = helpers.designed_arrays(**module.DESIGNED)
        assert len(arrays) == 7 and digest(arrays) == want, module.__name__
    v, cb, e, prob, B, lengths, v2snp = pair_shares_restatement.designed_problem()
    assert B == 48 and digest([v, cb, e, prob, v2snp, lengths]) == PAIR_SHARES_DIGEST
    for seed_base, of_length in GRID_DIGESTS.items():
        for n, want in of_length.items():
            assert digest([helpers.designed_grid(n, seed_base)]) == want, (seed_base, n)
    assert helpers.designed_grid(5).tobytes() == helpers.designed_grid(5, 100).tobytes(), 'the default is the ambient grids\' draw'
