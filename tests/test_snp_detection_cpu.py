"""SNP detection without a GPU: a vectorised numpy restatement of the contract (demuxalot_amd/snp_detection.py,
include/demux_hip.h "SNP detection") checked against the reference's captured outputs (tests/golden/f8_snp_*.npz, written
by make_snp_fixtures.py), the parquet export, and argument validation.  tests/test_gpu_snp_detection.py checks the device
against the same restatement."""
import numpy as np
import pandas as pd
import pytest

from tests import fixture_io as fio

P_BELOW = np.float32(0.01)


def flat_calls(candidate_calls, parts=None):
    """(chrom number, position, base, barcode, p) of every call, in container order.  `parts`: an explicit list of
    (chrom number, CompressedSNPCalls) instead of the dict, whose containers are numbered 0, 1, 2, ... in its order."""
    if parts is None:
        parts = list(enumerate(candidate_calls.values()))
    cols = [[], [], [], [], []]
    for k, calls in parts:
        sc = calls.snp_calls[:calls.n_snp_calls]
        mol = calls.molecules[:calls.n_molecules]
        cols[0].append(np.full(len(sc), k, dtype=np.int64))
        cols[1].append(sc['snp_position'].astype(np.int64))
        cols[2].append(sc['base_index'].astype(np.int64))
        cols[3].append(mol['compressed_cb'][sc['molecule_index']].astype(np.int64))
        cols[4].append(sc['p_base_wrong'])
    return [np.concatenate(c) if c else np.zeros(0, dtype=np.float32 if i == 4 else np.int64) for i, c in enumerate(cols)]


def count(candidate_calls, donor_of_barcode, n_donors, cap=3, parts=None, p_below=P_BELOW):
    """(chrom int32[P], pos int32[P], counts int32[P, D, 4]) in the canonical order: chrom value, then position; parts of
    equal chrom merge.  `parts` as for flat_calls; `p_below`: the threshold, compared in float32."""
    chrom, pos, base, cb, p = flat_calls(candidate_calls, parts)
    donor_of_barcode = np.asarray(donor_of_barcode)
    keep = (p < np.float32(p_below)) & (base < 4) & (donor_of_barcode[cb] >= 0)
    chrom, pos, base, cb = chrom[keep], pos[keep], base[keep], cb[keep]
    pos_key = chrom << 32 | (pos + 2 ** 31)
    positions, rank = np.unique(pos_key, return_inverse=True)
    B = len(donor_of_barcode)
    keys, runs = np.unique((rank * 4 + base) * B + cb, return_counts=True)
    counts = np.zeros((len(positions), n_donors, 4), dtype=np.int64)
    np.add.at(counts, (keys // (4 * B), donor_of_barcode[keys % B], (keys // B) % 4), np.minimum(runs, cap))
    return (positions >> 32).astype(np.int32), ((positions & 0xFFFFFFFF) - 2 ** 31).astype(np.int32), counts.astype(np.int32)


def score(counts, regularization=3.):
    """(importances float64[P, D], bases uint8[P, 2] (ref, alt), totals int64[P, 2])."""
    P, D, _ = counts.shape
    totals = counts.sum(axis=1, dtype=np.int64)
    order = np.argsort(totals, axis=1, kind='stable')
    alt, ref = order[:, -2], order[:, -1]
    rows = np.arange(P)
    c0 = counts[rows, :, alt] + 1e-4
    c1 = counts[rows, :, ref] + 1e-4
    s0, s1 = c0[:, 0].copy(), c1[:, 0].copy()
    for d in range(1, D):
        s0 = s0 + c0[:, d]
        s1 = s1 + c1[:, d]
    p_avg = (s1 / (s1 + s0))[:, None]
    p1 = (c1 + p_avg * regularization) / ((c0 + c1) + regularization)
    importances = np.square(p_avg - p1)
    bases = np.stack([ref, alt], axis=1).astype(np.uint8)
    return importances, bases, np.stack([totals[rows, ref], totals[rows, alt]], axis=1)


def select(importances, n_best, n_additional, row_sum=None):
    """_select_top_snps with stable rankings: selected indices, ascending.  `row_sum`: what stands in for
    importances.sum(axis=1) (tests/snp_detection_problems.py: the wrong associations)."""
    if n_best:
        best_for_donors = np.argsort(-importances, axis=0, kind='stable')[:n_best]
    else:  # (what [:0] leaves of the sort, without sorting)
        best_for_donors = np.zeros((0, importances.shape[1]), dtype=np.intp)
    overall = np.argsort(-(importances.sum(axis=1) if row_sum is None else row_sum(importances)), kind='stable')
    is_new = ~np.isin(overall, best_for_donors)
    overall = overall[:np.searchsorted(np.cumsum(is_new), n_additional, side='right')]
    return np.union1d(best_for_donors.flatten(), overall).astype(np.int64)


def donor_map(fx, prefix=''):
    barcodes = [str(b) for b in fx[f'{prefix}assign_barcodes']]
    donors = [str(d) for d in fx[f'{prefix}assign_donors']]
    return dict(zip(barcodes, donors))


def donor_index(barcode2donor, ordered_barcodes):
    sorted_donors = np.unique(list(barcode2donor.values()))
    index = {d: i for i, d in enumerate(sorted_donors)}
    return sorted_donors, np.asarray([index[barcode2donor[b]] if b in barcode2donor else -1 for b in ordered_barcodes],
                                     dtype=np.int32)


def known_calls(candidate_calls, genotypes):
    """The candidate containers restricted to the genotypes' positions (how the fixture's step-1 calls were made)."""
    from demuxalot_amd import CompressedSNPCalls
    positions = genotypes.get_chromosome2positions()
    out = {}
    for chrom, calls in candidate_calls.items():
        sc = calls.snp_calls[:calls.n_snp_calls]
        sc = sc[np.isin(sc['snp_position'], positions.get(chrom, np.zeros(0, dtype=int)))]
        c = CompressedSNPCalls(start_snps_size=1, start_molecule_size=1)
        c.molecules = calls.molecules[:calls.n_molecules].copy()
        c.n_molecules = calls.n_molecules
        c.snp_calls = sc.copy()
        c.n_snp_calls = len(sc)
        out[chrom] = c
    return out


def load(name):
    fx = fio.load(name)
    calls, genotypes, handler = fio.product_inputs(fx)
    return fx, calls, genotypes, handler


# --------------------------------------------------------------------------------------------------------------------
# the restatement against the reference
# --------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_reference_synthetic():
    fx, calls, _genotypes, handler = load('f8_snp_synthetic.npz')
    sorted_donors, dob = donor_index(donor_map(fx), handler.ordered_barcodes)
    assert list(sorted_donors) == [str(d) for d in fx['sorted_donors']]
    chrom, pos, counts = count(calls, dob, len(sorted_donors))
    assert np.array_equal(chrom, fx['all_chrom']) and np.array_equal(pos, fx['all_pos'])
    assert np.array_equal(counts, fx['all_counts'])
    importances, bases, totals = score(counts)
    fio.assert_bitwise(importances, fx['all_importances'], 'importances')
    assert np.array_equal(bases, fx['all_bases']) and np.array_equal(totals, fx['all_totals'])
    for s, (n_best, n_add, _ignore) in enumerate(fx['settings']):
        selected = select(importances, n_best, n_add)
        assert np.array_equal(chrom[selected], fx[f'sel{s}_chrom']) and np.array_equal(pos[selected], fx[f'sel{s}_pos'])


def _tied_top2(totals_all_bases):
    top = np.sort(totals_all_bases, axis=1)
    return top[:, -1] == top[:, -2]


@pytest.mark.parametrize('tag', ['three', 'one'])
def test_restatement_matches_reference_edge_cases(tag):
    """Cap exceeded, p == float32(0.01), tied base totals, unassigned barcodes, one donor, fewer positions than n_best.
    Where the top two base totals tie, the reference's pick follows whatever sort numpy dispatches to; the contract is a
    stable sort (ref = the higher base), so there the restatement stands alone."""
    fx, calls, _genotypes, handler = load('f8_snp_edge.npz')
    sorted_donors, dob = donor_index(donor_map(fx, f'{tag}_'), handler.ordered_barcodes)
    chrom, pos, counts = count(calls, dob, len(sorted_donors))
    assert np.array_equal(chrom, fx[f'{tag}_all_chrom']) and np.array_equal(pos, fx[f'{tag}_all_pos'])
    assert np.array_equal(counts, fx[f'{tag}_all_counts'])
    importances, bases, totals = score(counts)
    tied = _tied_top2(counts.sum(axis=1))
    assert tied.any()
    fio.assert_bitwise(importances[~tied], fx[f'{tag}_all_importances'][~tied], 'importances')
    assert np.array_equal(bases[~tied], fx[f'{tag}_all_bases'][~tied])
    assert np.array_equal(np.sort(totals, axis=1), np.sort(fx[f'{tag}_all_totals'], axis=1))
    for p in np.flatnonzero(tied):
        assert bases[p, 0] > bases[p, 1]  # the higher base is ref on a tie
    selected = select(importances, 100, 1000)
    assert np.array_equal(pos[selected], fx[f'{tag}_sel_pos'])


def test_edge_rules_by_hand():
    """The threshold compares in float32 (a stored 1e-2 is dropped), the cap applies per barcode, base N is dropped."""
    from demuxalot_amd import CompressedSNPCalls
    p = np.array([0.01, np.float32(0.01), 0.0099, 0.001, 0.001, 0.001, 0.001, 0.001, 0.001], dtype=np.float32)
    calls = {'c': CompressedSNPCalls.from_arrays([0, 1], [0, 0, 0, 1, 1, 1, 1, 1, 0], [5] * 8 + [6], [0, 0, 1, 2, 2, 2, 2, 2, 4], p)}
    chrom, pos, counts = count(calls, np.array([0, 0], dtype=np.int32), 1)
    assert list(pos) == [5]  # position 6 has an N call only
    assert counts[0, 0].tolist() == [0, 1, 3, 0]


# --------------------------------------------------------------------------------------------------------------------
# export and validation
# --------------------------------------------------------------------------------------------------------------------
def test_parquet_export_round_trips_through_add_prior_betas(tmp_path):
    from demuxalot_amd import ProbabilisticGenotypes
    from demuxalot_amd.snp_detection import export_snps_to_beta
    fx, calls, genotypes, _handler = load('f8_snp_synthetic.npz')
    chroms = [str(c) for c in fx['chroms']]
    bases = [str(b) for b in fx['detect0_bases']]
    selected = [(chroms[c], int(p), None, {bases[i][0]: 1, bases[i][1]: 1})
                for i, (c, p) in enumerate(zip(fx['detect0_chrom'], fx['detect0_pos']))]
    path = str(tmp_path / 'prior.parquet')
    export_snps_to_beta(selected, path)
    frame = pd.read_parquet(path)
    assert list(frame.columns) == [] and list(frame.index.names) == ['CHROM', 'POS', 'BASE']
    index = frame.index.to_frame()
    assert list(index['CHROM']) == [str(c) for c in fx['detect0_parquet_chrom']]
    assert list(index['POS']) == list(fx['detect0_parquet_pos'])
    assert list(index['BASE']) == [str(b) for b in fx['detect0_parquet_base']]
    before = genotypes.variant_betas[:genotypes.n_variants].copy()
    n_before = genotypes.n_variants
    genotypes.add_prior_betas(path)
    assert genotypes.n_variants == n_before + len(frame)
    for key in zip(index['CHROM'], index['POS'], index['BASE']):
        assert key in genotypes.var2varid
    fio.assert_bitwise(genotypes.variant_betas[:n_before], before, 'betas of the known variants')
    new_rows = genotypes.variant_betas[n_before:genotypes.n_variants]
    assert (new_rows == genotypes.default_prior).all() or np.isfinite(new_rows).all()
    # an empty selection writes an empty parquet
    export_snps_to_beta([], str(tmp_path / 'empty.parquet'))
    assert len(pd.read_parquet(str(tmp_path / 'empty.parquet'))) == 0


@pytest.mark.parametrize('kwargs, error', [
    (dict(n_best_snps_per_donor=-1), ValueError),
    (dict(n_best_snps_per_donor=2.5), ValueError),
    (dict(n_additional_best_snps=-3), ValueError),
    (dict(max_contribution_to_base_count_from_barcode=-1), ValueError),
    (dict(max_contribution_to_base_count_from_barcode=1.5), ValueError),
    (dict(regularization=float('nan')), ValueError),
    (dict(regularization=-1.), ValueError),
])
def test_argument_validation(kwargs, error):
    from demuxalot_amd import select_snps_from_calls
    _fx, calls, _genotypes, handler = load('f8_snp_edge.npz')
    with pytest.raises(error):
        select_snps_from_calls(calls, handler, {'BC00': 'D'}, **kwargs)


def test_argument_types():
    from demuxalot_amd import detect_snps_positions_from_calls, select_snps_from_calls
    _fx, calls, genotypes, handler = load('f8_snp_edge.npz')
    with pytest.raises(TypeError):
        select_snps_from_calls(list(calls.values()), handler, {'BC00': 'D'})
    with pytest.raises(TypeError):
        select_snps_from_calls(calls, handler, [('BC00', 'D')])
    with pytest.raises(ValueError):
        detect_snps_positions_from_calls(calls, calls, genotypes, handler, n_best_snps_per_donor=-1)


def test_no_assigned_barcode_is_an_empty_result(tmp_path):
    """No donor at all: nothing to count, an empty list (and an empty parquet), without touching a device."""
    from demuxalot_amd import select_snps_from_calls
    _fx, calls, _genotypes, handler = load('f8_snp_edge.npz')
    path = str(tmp_path / 'prior.parquet')
    assert select_snps_from_calls(calls, handler, {}, result_beta_prior_filename=path) == []
    assert len(pd.read_parquet(path)) == 0
