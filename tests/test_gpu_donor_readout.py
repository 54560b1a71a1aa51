"""Donor-level read-outs of the resident posteriors on the GPU (include/demux_hip_debug.h: dmx_get_donor_readout,
dmx_get_allowed_mass; DevicePosteriors.doublet_probability / donor_marginals / droplet_calls / donor_summary / qualities).

The checker is tests/donor_readout_restatement.py applied to get_probs() of the same context: donor marginals, arg-maxes and allowed
masses bit for bit (their order of additions is the contract), the two masses within a relative 2 K 2^-53 (each of two summation
orders of K non-negative float64 terms errs by at most (K - 1) 2^-53).  The frames are compared with the restatement applied to
the reference's own captured posteriors (golden fixtures)."""
import numpy as np
import pandas as pd
import pytest

from tests import donor_readout_restatement as restated
from tests import fixture_io as fio

pytestmark = pytest.mark.gpu

RAW_KEYS = ('singlet_mass', 'doublet_mass', 'best_singlet', 'best_singlet_prob', 'best_pair', 'best_pair_prob')


def assert_masses(got, want, K, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert (np.abs(got - want) <= 2 * K * 2.0 ** -53 * np.abs(want)).all(), (what, np.abs(got - want).max())


def assert_readout(got, P, G, what):
    """The raw arrays of get_donor_readout against the restatement on the float32 posteriors P."""
    want = restated.readout(P, G)
    K = P.shape[1]
    assert_masses(got['singlet_mass'], want['singlet_mass'], K, f'{what}: singlet mass')
    assert_masses(got['doublet_mass'], want['doublet_mass'], K, f'{what}: doublet mass')
    for key in ('best_singlet', 'best_pair'):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key)
        fio.assert_bitwise(got[key + '_prob'], want[key + '_prob'], f'{what}: {key}_prob')
    if 'donor_marginals' in got:
        fio.assert_bitwise(got['donor_marginals'], want['donor_marginals'], f'{what}: donor marginals')
    return want


def assert_same_calls(got, want, K, what):
    for column in ('status', 'donor_1', 'donor_2'):
        assert list(got[column]) == list(want[column]), (what, column)
    singlets = (want['status'] == 'singlet').values
    fio.assert_bitwise(got['probability'].values[singlets], want['probability'].values[singlets].astype(np.float64), f'{what}: singlet probability')
    assert_masses(got['probability'].values[~singlets], want['probability'].values[~singlets].astype(np.float64), K, f'{what}: probability')
    assert_masses(got['doublet_probability'].values, want['doublet_probability'].values.astype(np.float64), K, f'{what}: doublet probability')


# status counts at threshold 0.9 of the reference's captured posteriors: (fixture, predict) -> singlet, doublet, unassigned
KNOWN_COUNTS = {('f3_small_2.npz', 2): (1, 4, 35), ('f1_synthetic_default.npz', 1): (810, 190, 0)}


@pytest.mark.parametrize('name', ['f1_synthetic_default.npz', 'f3_small_2.npz', 'f3_small_4.npz', 'f6_shipped_example.npz'])
def test_read_outs_on_reference_posteriors(name):
    from demuxalot_amd import Demultiplexer
    fx = fio.load(name)
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    G = len(donors)
    for i in range(int(fx['n_predict'])):
        dp, clip = float(fx[f'predict{i}_dp']), float(fx[f'predict{i}_clip'])
        reference = fx[f'predict{i}_probs']
        K = reference.shape[1]
        what = f'{name} predict {i}'
        with Demultiplexer.predict_posteriors(calls, genotypes, handler, p_genotype_clip=clip, doublet_prior=dp, on_device=True) as dev:
            assert dev.n_donors == G and dev.donor_names == donors and dev.shape == reference.shape
            P = dev._ctx.get_probs()
            raw = dev._ctx.get_donor_readout(marginals=True)
            assert_readout(raw, P, G, what)
            lean = dev._ctx.get_donor_readout()
            assert 'donor_marginals' not in lean
            for key in RAW_KEYS:
                fio.assert_bitwise(lean[key], raw[key], f'{what}: {key} without marginals')

            want = restated.readout(reference, G)
            marginals = dev.donor_marginals()
            assert list(marginals.columns) == donors and list(marginals.index) == handler.ordered_barcodes
            assert marginals.index.name == 'BARCODE' and marginals.values.dtype == np.float32
            fio.assert_bitwise(marginals.values, want['donor_marginals'], f'{what}: donor_marginals()')
            if dp == 0:
                fio.assert_bitwise(marginals.values, reference, f'{what}: without doublets the marginals are the posteriors')
            doublet_probability = dev.doublet_probability()
            assert doublet_probability.dtype == np.float64 and list(doublet_probability.index) == handler.ordered_barcodes
            assert_masses(doublet_probability.values, want['doublet_mass'], K, f'{what}: doublet_probability()')
            if dp == 0:
                assert not doublet_probability.values.any()
            for thr in (0.9, 0.5, 0.999999):
                got = dev.droplet_calls(thr)
                want_calls = restated.calls(reference, donors, thr)
                assert list(got.index) == handler.ordered_barcodes and got.index.name == 'BARCODE'
                assert_same_calls(got, want_calls, K, f'{what} at {thr}')
                if dp == 0:
                    assert 'doublet' not in set(got['status'])
                if thr == 0.9 and (name, i) in KNOWN_COUNTS:
                    counts = tuple(int((got['status'] == s).sum()) for s in ('singlet', 'doublet', 'unassigned'))
                    assert counts == KNOWN_COUNTS[name, i], (what, counts)
                summary = dev.donor_summary(thr)
                want_summary = restated.summary(reference, donors, thr)
                assert list(summary.index) == donors and list(summary.columns) == ['n_singlets', 'n_doublets', 'expected_cells']
                assert list(summary['n_singlets']) == list(want_summary['n_singlets']), (what, thr)
                assert list(summary['n_doublets']) == list(want_summary['n_doublets']), (what, thr)
                assert summary['expected_cells'].dtype == np.float64
                assert np.allclose(summary['expected_cells'], want_summary['expected_cells'], rtol=1e-12, atol=0), (what, thr)


def random_context(B, G, with_doublets, V=50, seed=0):
    """A raw context with a few hundred random calls, a random table in [0, 1) and one E-step behind it."""
    from demuxalot_amd.device import DeviceContext
    rng = np.random.default_rng([seed, B, G])
    n_calls = 8 * B
    ctx = DeviceContext(0)
    try:
        ctx.set_problem(B, V, G, rng.integers(0, V, n_calls), rng.integers(0, max(B, 1), n_calls),
                        rng.uniform(0.001, 0.3, n_calls).astype(np.float32), np.arange(V, dtype=np.int32) // 2)
        ctx.set_probs(rng.random((V, G), dtype=np.float32))
        K = G * (G + 1) // 2 if with_doublets else G
        ctx.estep(np.zeros(K, dtype=np.float32), with_doublets=with_doublets, fetch_logits=False, fetch_probs=False)
    except BaseException:
        ctx.close()
        raise
    return ctx


# G <= 64: a wavefront per barcode with the row in LDS; up to 8448 columns: a workgroup per barcode with the row in LDS; beyond:
# a workgroup per barcode reading global memory.  B = 37 is no multiple of the four barcodes of a workgroup.
@pytest.mark.parametrize('B,G,with_doublets', [
    (37, 1, False), (37, 2, True), (37, 3, True), (37, 5, False), (37, 64, True), (37, 65, True), (37, 128, True), (37, 129, True),
    (1, 3, True), (1, 65, True), (37, 1, True), (37, 70, False)])
def test_raw_read_out_at_the_kernel_forms_edges(B, G, with_doublets):
    ctx = random_context(B, G, with_doublets)
    try:
        P = ctx.get_probs()
        assert P.shape == (B, G * (G + 1) // 2 if with_doublets else G)
        got = ctx.get_donor_readout(marginals=True)
        assert got['donor_marginals'].shape == (B, G)
        want = assert_readout(got, P, G, f'B={B} G={G} doublets={with_doublets}')
        if P.shape[1] == G:
            assert (got['best_pair'] == -1).all() and np.isnan(got['best_pair_prob']).all() and not got['doublet_mass'].any()
            fio.assert_bitwise(got['donor_marginals'], P, 'no pair columns: the marginals are the posteriors')
        else:
            assert (got['best_pair'] >= G).all()
        lean = ctx.get_donor_readout()  # donor_marginals = NULL: another kernel form, the same other outputs
        assert 'donor_marginals' not in lean
        for key in RAW_KEYS:
            fio.assert_bitwise(lean[key], got[key], f'{key} without marginals')
        assert np.array_equal(want['best_singlet'], np.argmax(P[:, :G], axis=1))
    finally:
        ctx.close()


def test_no_barcodes():
    ctx = random_context(0, 3, True)
    try:
        got = ctx.get_donor_readout(marginals=True)
        assert got['donor_marginals'].shape == (0, 3) and all(len(got[key]) == 0 for key in RAW_KEYS)
        mass, hit = ctx.get_allowed_mass(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        assert mass.shape == (0,) and hit.shape == (0,)
    finally:
        ctx.close()


def test_ties_go_to_the_lower_column():
    """The equal-evidence problem of test_gpu_results' tie test, with doublets: every option of a barcode has the same logit."""
    from demuxalot_amd.device import DeviceContext
    ctx = DeviceContext(0)
    try:
        ctx.set_problem(3, 2, 2, np.array([0, 1, 0]), np.array([0, 1, 2]), np.full(3, .1, dtype='f4'), np.zeros(2, dtype='i4'))
        ctx.set_probs(np.full((2, 2), 0.5, dtype=np.float32))
        _, probs = ctx.estep(np.zeros(3, dtype=np.float32), with_doublets=True)
        assert probs.shape == (3, 3) and (probs[:, :1] == probs).all(), 'equal evidence: equal posteriors'
        got = ctx.get_donor_readout(marginals=True)
        assert got['best_singlet'].tolist() == [0, 0, 0] and got['best_pair'].tolist() == [2, 2, 2]
        assert_readout(got, probs, 2, 'ties')
        mass, hit = ctx.get_allowed_mass([0, 1, 2, 3], [0, 1, 2])  # the first maximum is column 0, whatever equals it
        assert hit.tolist() == [1, 0, 0]
        fio.assert_bitwise(mass, probs[[0, 1, 2], [0, 1, 2]].astype(np.float64), 'tied masses')
    finally:
        ctx.close()


def test_allowed_mass_lists_and_refused_inputs():
    from demuxalot_amd import _lib
    B, G = 37, 5
    ctx = random_context(B, G, True, seed=1)
    try:
        P = ctx.get_probs()
        K = P.shape[1]
        top = np.argmax(P, axis=1)
        lists = []
        for b in range(B):  # lengths 0, 1 and 3; with and without the arg-max; repeated options
            other = [(int(top[b]) + s) % K for s in (1, 2, 3)]
            lists.append([[], [int(top[b])], [other[0]], [other[0], int(top[b]), other[1]], other, [other[2], other[2], other[0]],
                          [int(top[b])] * 3][b % 7])
        start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        options = np.asarray([k for x in lists for k in x], dtype=np.int32)
        mass, hit = ctx.get_allowed_mass(start, options)
        want_mass, want_hit = restated.allowed_mass(P, start, options)
        fio.assert_bitwise(mass, want_mass, 'allowed mass')
        assert hit.dtype == np.int32 and np.array_equal(hit, want_hit)
        assert set(hit.tolist()) == {0, 1} and hit[0] == 0 and mass[0] == 0.0
        with pytest.raises(_lib.DemuxHipError, match='dmx_get_allowed_mass'):  # an option >= K
            bad = options.copy()
            bad[5] = K
            ctx.get_allowed_mass(start, bad)
        with pytest.raises(_lib.DemuxHipError, match='dmx_get_allowed_mass'):  # a negative option
            bad = options.copy()
            bad[0] = -1
            ctx.get_allowed_mass(start, bad)
        with pytest.raises(_lib.DemuxHipError, match='decreases'):
            bad = start.copy()
            bad[3] = bad[2] - 1
            ctx.get_allowed_mass(bad, options)
        with pytest.raises(_lib.DemuxHipError, match=r'allowed_start\[0\]'):
            ctx.get_allowed_mass(start + 1, np.concatenate([options, [0]]).astype(np.int32))
        again, _ = ctx.get_allowed_mass(start, options)  # the refusals left the context usable
        fio.assert_bitwise(again, want_mass, 'allowed mass after refusals')
    finally:
        ctx.close()


def test_qualities_on_reference_posteriors():
    from demuxalot_amd import Demultiplexer
    fx = fio.load('f1_synthetic_default.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    reference = fx['predict1_probs']
    columns = [str(c) for c in fx['predict1_columns']]
    K = len(columns)
    frame = pd.DataFrame(reference, index=handler.ordered_barcodes, columns=columns)
    top = reference.argmax(axis=1)
    # every barcode is allowed its most probable option and two others; in the second dict every third barcode loses the first
    allowed = {b: [columns[(t + 7) % K], columns[t], columns[(t + 13) % K]] for b, t in zip(handler.ordered_barcodes, top)}
    harder = {b: names[::2] if i % 3 == 0 else names for i, (b, names) in enumerate(allowed.items())}
    with Demultiplexer.predict_posteriors(calls, genotypes, handler, p_genotype_clip=float(fx['predict1_clip']),
                                          doublet_prior=float(fx['predict1_dp']), on_device=True) as dev:
        assert dev.columns == columns
        for possible in (allowed, harder):
            got = dev.qualities(possible)
            assert set(got) == {'logloss', 'accuracy', 'error rate'}
            want64, want32 = restated.qualities_float64(frame, possible), restated.qualities_pandas_float32(frame, possible)
            assert got['accuracy'] == want64['accuracy'] == want32['accuracy']
            assert got['error rate'] == 1 - got['accuracy']
            assert np.isclose(got['logloss'], want64['logloss'], rtol=1e-12, atol=0)
            assert np.isclose(got['logloss'], want32['logloss'], rtol=2e-5, atol=0)  # pandas adds in float32
        assert dev.qualities(allowed)['accuracy'] == 1.0 and dev.qualities(harder)['accuracy'] < 1.0
        with pytest.raises(ValueError):
            dev.qualities({b: allowed[b] for b in handler.ordered_barcodes[1:]})


def test_learn_genotypes_on_device_has_the_read_outs():
    from demuxalot_amd import Demultiplexer
    fx = fio.load('f3_small_2.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    for dp in (0.0, 0.25):
        _learnt, dev = Demultiplexer.learn_genotypes(calls, genotypes, handler, n_iterations=2, doublet_prior=dp, on_device=True)
        with dev:
            P = dev._ctx.get_probs()
            G = genotypes.n_genotypes
            assert dev.n_donors == G and P.shape[1] == (G if dp == 0 else G * (G + 1) // 2)
            fio.assert_bitwise(dev.donor_marginals().values, restated.readout(P, G)['donor_marginals'], 'marginals after EM')
            got = dev.droplet_calls(0.5)
            assert_same_calls(got, restated.calls(P, dev.donor_names, 0.5), P.shape[1], f'calls after EM, dp={dp}')
            assert got.index.name is None and list(got.index) == handler.ordered_barcodes


def test_call_order():
    from demuxalot_amd import _lib
    from demuxalot_amd.device import DeviceContext
    ctx = DeviceContext(0)
    try:
        ctx.set_problem(3, 2, 2, np.array([0, 1, 0]), np.array([0, 1, 2]), np.full(3, .1, dtype='f4'), np.zeros(2, dtype='i4'))
        ctx.set_probs(np.full((2, 2), 0.5, dtype=np.float32))
        with pytest.raises(_lib.DemuxHipError, match='dmx_get_donor_readout'):
            ctx.get_donor_readout()
        with pytest.raises(_lib.DemuxHipError, match='dmx_get_allowed_mass'):
            ctx.get_allowed_mass(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32))
    finally:
        ctx.close()
