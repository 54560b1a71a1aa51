"""Host side of the donor-level read-outs (demuxalot_amd/donor_readout.py, DevicePosteriors' argument checks): runs without a GPU."""
import numpy as np
import pytest

from tests import donor_readout_restatement as restated


@pytest.mark.parametrize('G', [1, 2, 3, 64, 65, 128])
def test_column_pair_mapping_round_trip(G):
    """Columns <-> (g1, g2) against the enumeration order of _option_names."""
    from demuxalot_amd import donor_readout
    from demuxalot_amd.demux import _option_names
    names = [f'd{g}' for g in range(G)]
    columns = _option_names(names, 0.35)
    assert len(columns) == donor_readout.n_options(G, True) and donor_readout.n_options(G, False) == G
    g1, g2 = donor_readout.column_donors(G, np.arange(len(columns)))
    want = [names[a] if b < 0 else f'{names[a]}+{names[b]}' for a, b in zip(g1, g2)]
    assert want == columns
    assert (g2[:G] == -1).all() and (g1[:G] == np.arange(G)).all()
    if G > 1:
        assert np.array_equal(donor_readout.pair_column(G, g1[G:], g2[G:]), np.arange(G, len(columns)))
    assert [tuple(int(x) for x in pair if x >= 0) for pair in zip(g1, g2)] == restated.enumerate_options(G, True)
    assert donor_readout.column_donors(G, [-1]) == (-1, -1)
    for g in {0, G // 2, G - 1}:
        assert list(donor_readout.donor_columns(G, g, True)) == [k for k, c in enumerate(columns) if names[g] in c.split('+')]
        assert list(donor_readout.donor_columns(G, g, False)) == [g]


def test_droplet_calls_composition_strictness_and_precedence():
    from demuxalot_amd import donor_readout
    names = ['A', 'B', 'C']  # columns: A B C A+B A+C B+C
    thr = np.float32(0.9)
    above32, above64 = np.nextafter(thr, np.float32(1)), np.nextafter(np.float64(0.9), 1.0)
    got = donor_readout.compose_calls(
        names, 0.9,
        best_singlet=np.array([1, 1, 2, 2, 0], dtype=np.int32),
        best_singlet_prob=np.array([thr, above32, 0.05, 0.05, 0.3], dtype=np.float32),
        best_pair=np.array([3, 3, 5, 4, 4], dtype=np.int32),
        doublet_mass=np.array([0.05, 0.05, 0.9, above64, 0.6]), index=list('vwxyz'))
    assert list(got.columns) == ['status', 'donor_1', 'donor_2', 'probability', 'doublet_probability']
    assert list(got.index) == list('vwxyz')
    # float32(0.9) is not > float32(0.9); its successor is.  float64 0.9 is not > 0.9; its successor is.
    assert list(got['status']) == ['unassigned', 'singlet', 'unassigned', 'doublet', 'unassigned']
    assert list(got['donor_1']) == [None, 'B', None, 'A', None]
    assert list(got['donor_2']) == [None, None, None, 'C', None]
    assert got['probability'].dtype == np.float64 and got['doublet_probability'].dtype == np.float64
    assert list(got['probability']) == [float(thr), float(above32), 0.9, above64, 0.6]
    assert list(got['doublet_probability']) == [0.05, 0.05, 0.9, above64, 0.6]
    # float32(0.1) widened is above float64 0.1: the singlet comparison is the float32 one (Series.gt on a float32 column), in which
    # float32(0.1) is not > 0.1; the doublet comparison is the float64 one, in which the same number is
    tenth = np.float32(0.1)
    assert float(tenth) > 0.1
    edge = donor_readout.compose_calls(names, 0.1, np.array([0, 0]), np.array([tenth, 0.0], dtype=np.float32), np.array([3, 3]),
                                       np.array([0.0, float(tenth)]))
    assert list(edge['status']) == ['unassigned', 'doublet']
    # threshold below one half: both a singlet and the doublet mass can be above it; the singlet wins
    low = donor_readout.compose_calls(names, 0.4, np.array([2, 2]), np.array([0.45, 0.3], dtype=np.float32), np.array([3, 3]),
                                      np.array([0.5, 0.65]))
    assert list(low['status']) == ['singlet', 'doublet']
    assert list(low['donor_1']) == ['C', 'A'] and list(low['donor_2']) == [None, 'B']
    assert list(low['probability']) == [float(np.float32(0.45)), 0.65]


def test_droplet_calls_composition_without_pair_columns():
    from demuxalot_amd import donor_readout
    got = donor_readout.compose_calls(['A', 'B'], 0.9, np.array([0, 1], dtype=np.int32), np.array([0.95, 0.6], dtype=np.float32),
                                      np.array([-1, -1], dtype=np.int32), np.zeros(2))
    assert list(got['status']) == ['singlet', 'unassigned']
    assert list(got['donor_1']) == ['A', None] and list(got['donor_2']) == [None, None]
    assert list(got['probability']) == [float(np.float32(0.95)), float(np.float32(0.6))]
    assert list(got['doublet_probability']) == [0.0, 0.0]
    # a threshold below 0 must not turn the absent pairs into a doublet
    assert 'doublet' not in set(donor_readout.compose_calls(['A'], -1.0, np.array([0]), np.array([np.nan], dtype=np.float32),
                                                            np.array([-1]), np.zeros(1))['status'])


def test_composition_matches_the_restatement_on_random_posteriors():
    from demuxalot_amd import donor_readout
    rng = np.random.default_rng(3)
    names = ['a', 'b', 'c', 'd']
    P = rng.dirichlet(np.full(10, 0.15), size=200).astype(np.float32)
    r = restated.readout(P, 4)
    for thr in (0.3, 0.5, 0.9):
        got = donor_readout.compose_calls(names, thr, r['best_singlet'], r['best_singlet_prob'], r['best_pair'], r['doublet_mass'])
        want = restated.calls(P, names, thr)
        assert set(want['status']) == ({'singlet', 'doublet', 'unassigned'} if thr >= 0.5 else {'singlet', 'doublet'})
        for column in want.columns:
            assert list(got[column]) == list(want[column]), (thr, column)
        summary = donor_readout.compose_summary(names, got, P.astype(np.float64).sum(axis=0))
        want_summary = restated.summary(P, names, thr)
        assert list(summary.index) == names and summary.index.name == 'donor'
        assert list(summary['n_singlets']) == list(want_summary['n_singlets'])
        assert list(summary['n_doublets']) == list(want_summary['n_doublets'])
        assert np.allclose(summary['expected_cells'], want_summary['expected_cells'], rtol=1e-14, atol=0)
        assert np.allclose(summary['expected_cells'], r['donor_marginals'].astype(np.float64).sum(axis=0), rtol=1e-6, atol=0)


def test_expected_cells_from_hand_made_option_sums():
    from demuxalot_amd import donor_readout
    # A B C A+B A+C B+C
    sums = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    assert list(donor_readout.expected_cells(3, sums)) == [1 + 8 + 16, 2 + 8 + 32, 4 + 16 + 32]
    assert list(donor_readout.expected_cells(3, sums[:3])) == [1.0, 2.0, 4.0]  # no doublets: the donor's own column
    calls = donor_readout.compose_calls(['A', 'B', 'C'], 0.9, np.array([0, 0]), np.array([0.95, 0.01], dtype=np.float32),
                                        np.array([5, 5]), np.array([0.0, 0.98]))
    summary = donor_readout.compose_summary(['A', 'B', 'C'], calls, sums)
    assert list(summary.columns) == ['n_singlets', 'n_doublets', 'expected_cells']
    assert list(summary['n_singlets']) == [1, 0, 0] and list(summary['n_doublets']) == [0, 1, 1]
    assert list(summary['expected_cells']) == [25.0, 42.0, 52.0] and summary['expected_cells'].dtype == np.float64
    with pytest.raises(AssertionError):
        donor_readout.expected_cells(3, sums[:5])


def test_qualities_argument_errors():
    """A barcode missing from the dict and a name that is not a column: ValueError, before anything touches the device."""
    from demuxalot_amd import DevicePosteriors, donor_readout
    dev = DevicePosteriors(None, ['b0', 'b1'], ['A', 'B', 'A+B'], n_donors=2)
    assert dev.donor_names == ['A', 'B'] and dev.n_donors == 2
    with pytest.raises(ValueError, match='b1'):
        dev.qualities({'b0': ['A']})
    with pytest.raises(ValueError, match='B\\+A'):
        dev.qualities({'b0': ['A'], 'b1': ['B+A']})
    with pytest.raises(ValueError, match='Z'):  # the reference checks every entry of the dict, used or not
        dev.qualities({'b0': ['A'], 'b1': ['B'], 'elsewhere': ['Z']})
    start, options = donor_readout.allowed_lists(['b0', 'b1'], ['A', 'B', 'A+B'], {'b1': [], 'b0': ['A+B', 'A', 'A+B'], 'more': ['B']})
    assert start.dtype == np.int64 and options.dtype == np.int32
    assert list(start) == [0, 3, 3] and list(options) == [2, 0, 2]
    q = donor_readout.compose_qualities(np.array([0.5, 0.0, 1.0]), np.array([1, 0, 1], dtype=np.int32))
    assert q['logloss'] == np.mean([-np.log(0.5), -np.log(1e-4), 0.0])
    assert q['accuracy'] == 2 / 3 and q['error rate'] == 1 - 2 / 3


def test_qualities_host_path_on_restated_device_arrays():
    """allowed_lists -> (the device pass, restated) -> compose_qualities against the two restatements of the reference's formula."""
    import pandas as pd
    from demuxalot_amd import donor_readout
    rng = np.random.default_rng(4)
    columns = ['A', 'B', 'C', 'A+B', 'A+C', 'B+C']
    P = rng.dirichlet(np.full(6, 0.3), size=50).astype(np.float32)
    frame = pd.DataFrame(P, index=[f'b{i}' for i in range(50)], columns=columns)
    possible = {b: [columns[i % 6], columns[(i + 2) % 6]] for i, b in enumerate(frame.index)}
    q64, q32 = restated.qualities_float64(frame, possible), restated.qualities_pandas_float32(frame, possible)
    assert q64['accuracy'] == q32['accuracy'] and 0 < q64['accuracy'] < 1
    assert np.isclose(q64['logloss'], q32['logloss'], rtol=2e-5, atol=0)
    start, options = donor_readout.allowed_lists(list(frame.index), columns, possible)
    got = donor_readout.compose_qualities(*restated.allowed_mass(P, start, options))
    assert got['accuracy'] == q64['accuracy'] and got['error rate'] == q64['error rate']
    assert np.isclose(got['logloss'], q64['logloss'], rtol=1e-14, atol=0)
