"""SNP detection on the GPU (include/demux_hip.h "SNP detection", demuxalot_amd/snp_detection.py): counts, importances,
bases and selections against the reference's captured outputs (tests/golden/f8_snp_*.npz) and against the numpy
restatement of tests/test_snp_detection_cpu.py on random problems full of ties and one large skewed problem; the end-to-end
detect_snps_positions_from_calls against the reference's detect_snps_positions; coexistence with a DevicePosteriors."""
import numpy as np
import pandas as pd
import pytest

from tests import fixture_io as fio
from tests import test_snp_detection_cpu as r

pytestmark = pytest.mark.gpu


def _context():
    from demuxalot_amd.device import get_context
    return get_context()


def _device_run(ctx, calls, dob, n_donors, reg=3., cap=3, n_best=100, n_add=1000):
    from demuxalot_amd.snp_detection import P_BASE_WRONG_BELOW, _containers
    n = ctx.snp_count(_containers(calls), dob, n_donors, P_BASE_WRONG_BELOW, cap)
    scored = ctx.snp_score(reg)
    assert len(scored['pos']) == n
    return scored, ctx.snp_select(n_best, n_add)


def _check_against_restatement(scored, selected, calls, dob, n_donors, reg=3., cap=3, n_best=100, n_add=1000):
    chrom, pos, counts = r.count(calls, dob, n_donors, cap)
    assert np.array_equal(scored['chrom'], chrom) and np.array_equal(scored['pos'], pos)
    assert np.array_equal(scored['counts'], counts)
    importances, bases, totals = r.score(counts, reg)
    fio.assert_bitwise(scored['importances'], importances, 'importances')
    assert np.array_equal(scored['bases'], bases) and np.array_equal(scored['base_totals'], totals)
    assert np.array_equal(selected, r.select(importances, n_best, n_add))


def test_fixture_counts_importances_selection():
    fx, calls, _genotypes, handler = r.load('f8_snp_synthetic.npz')
    sorted_donors, dob = r.donor_index(r.donor_map(fx), handler.ordered_barcodes)
    ctx = _context()
    for s, (n_best, n_add, _ignore) in enumerate(fx['settings']):
        scored, selected = _device_run(ctx, calls, dob, len(sorted_donors), n_best=n_best, n_add=n_add)
        assert np.array_equal(scored['chrom'], fx['all_chrom']) and np.array_equal(scored['pos'], fx['all_pos'])
        assert np.array_equal(scored['counts'], fx['all_counts'])
        fio.assert_bitwise(scored['importances'], fx['all_importances'], 'importances')
        assert np.array_equal(scored['bases'], fx['all_bases']) and np.array_equal(scored['base_totals'], fx['all_totals'])
        assert np.array_equal(scored['chrom'][selected], fx[f'sel{s}_chrom'])
        assert np.array_equal(scored['pos'][selected], fx[f'sel{s}_pos'])


@pytest.mark.parametrize('tag', ['three', 'one'])
def test_fixture_edge_cases(tag):
    fx, calls, _genotypes, handler = r.load('f8_snp_edge.npz')
    sorted_donors, dob = r.donor_index(r.donor_map(fx, f'{tag}_'), handler.ordered_barcodes)
    scored, selected = _device_run(_context(), calls, dob, len(sorted_donors))
    assert np.array_equal(scored['counts'], fx[f'{tag}_all_counts'])
    assert np.array_equal(scored['pos'][selected], fx[f'{tag}_sel_pos'])
    _check_against_restatement(scored, selected, calls, dob, len(sorted_donors))


def test_select_snps_from_calls_fixture():
    from demuxalot_amd import select_snps_from_calls
    fx, calls, genotypes, handler = r.load('f8_snp_synthetic.npz')
    chroms = [str(c) for c in fx['chroms']]
    barcode2donor = r.donor_map(fx)
    for s, (n_best, n_add, ignore) in enumerate(fx['settings']):
        for mapping in (barcode2donor, pd.Series(barcode2donor)):
            result = select_snps_from_calls(calls, handler, mapping, n_best_snps_per_donor=int(n_best),
                                            n_additional_best_snps=int(n_add), genotypes=genotypes, ignore_known_snps=bool(ignore))
            assert [(c, p) for c, p, *_ in result] == [(chroms[c], int(p)) for c, p in zip(fx[f'detect{s}_chrom'], fx[f'detect{s}_pos'])]
            fio.assert_bitwise(np.stack([imp for _, _, imp, _ in result]), fx[f'detect{s}_importances'], 'importances')
            assert [''.join(bc) for *_, bc in result] == [str(b) for b in fx[f'detect{s}_bases']]
            assert np.array_equal([list(bc.values()) for *_, bc in result], fx[f'detect{s}_totals'])


@pytest.mark.parametrize('s', [0, 1, 2])
def test_detect_snps_positions_from_calls_end_to_end(s, tmp_path):
    from demuxalot_amd import detect_snps_positions_from_calls
    fx, calls, genotypes, handler = r.load('f8_snp_synthetic.npz')
    chroms = [str(c) for c in fx['chroms']]
    n_best, n_add, ignore = fx['settings'][s]
    path = str(tmp_path / 'prior.parquet')
    result = detect_snps_positions_from_calls(r.known_calls(calls, genotypes), calls, genotypes, handler,
                                              n_best_snps_per_donor=int(n_best), n_additional_best_snps=int(n_add),
                                              ignore_known_snps=bool(ignore), result_beta_prior_filename=path)
    assert [(c, p) for c, p, *_ in result] == [(chroms[c], int(p)) for c, p in zip(fx[f'detect{s}_chrom'], fx[f'detect{s}_pos'])]
    fio.assert_bitwise(np.stack([imp for _, _, imp, _ in result]), fx[f'detect{s}_importances'], 'importances')
    assert [''.join(bc) for *_, bc in result] == [str(b) for b in fx[f'detect{s}_bases']]
    assert np.array_equal([list(bc.values()) for *_, bc in result], fx[f'detect{s}_totals'])
    index = pd.read_parquet(path).index.to_frame()
    assert list(index['CHROM']) == [str(c) for c in fx[f'detect{s}_parquet_chrom']]
    assert list(index['POS']) == list(fx[f'detect{s}_parquet_pos'])
    assert list(index['BASE']) == [str(b) for b in fx[f'detect{s}_parquet_base']]
    # recovery of the true SNPs hidden from the genotypes: what the reference recovers
    hidden = {(chroms[c], int(p)) for c, p, h in zip(fx['true_chrom'], fx['true_pos'], fx['true_hidden']) if h}
    assert len({(c, p) for c, p, *_ in result} & hidden) == int(fx[f'detect{s}_recovered'])


def _random_calls(rng, n_chrom, n_calls, n_barcodes, n_positions, skew=False):
    from demuxalot_amd import CompressedSNPCalls
    calls = {}
    for k in range(n_chrom):
        n = n_calls // n_chrom
        n_mol = max(1, n // 3)
        mol_cb = rng.integers(0, n_barcodes, n_mol).astype(np.int32)
        if skew:  # a few positions carry most of the coverage
            pos = (rng.zipf(1.3, n) % n_positions).astype(np.int32) * 7 + 11
        else:
            pos = rng.integers(0, n_positions, n).astype(np.int32) * 3
        base = rng.choice(5, n, p=[0.35, 0.3, 0.15, 0.15, 0.05]).astype(np.uint8)
        p = rng.choice(np.asarray([0.001, 0.005, np.float32(0.01), 0.02, 0.0099], dtype=np.float32), n, p=[0.5, 0.2, 0.1, 0.1, 0.1])
        calls[f'chr{k}'] = CompressedSNPCalls.from_arrays(mol_cb, rng.integers(0, n_mol, n).astype(np.int32), pos, base, p)
    return calls


@pytest.mark.parametrize('seed, n_chrom, n_calls, n_barcodes, n_positions, n_donors, n_best, n_add, cap', [
    (0, 1, 300, 12, 20, 1, 3, 2, 3),
    (1, 3, 5000, 40, 60, 3, 5, 7, 3),
    (2, 2, 20000, 300, 500, 17, 10, 30, 2),
    (3, 4, 50000, 2000, 3000, 8, 0, 40, 5),
    (4, 2, 30000, 100, 1000, 64, 4, 0, 1),
])
def test_random_problems_with_ties(seed, n_chrom, n_calls, n_barcodes, n_positions, n_donors, n_best, n_add, cap):
    rng = np.random.default_rng(seed)
    calls = _random_calls(rng, n_chrom, n_calls, n_barcodes, n_positions)
    dob = rng.integers(-1, n_donors, n_barcodes).astype(np.int32)
    scored, selected = _device_run(_context(), calls, dob, n_donors, reg=3., cap=cap, n_best=n_best, n_add=n_add)
    _check_against_restatement(scored, selected, calls, dob, n_donors, reg=3., cap=cap, n_best=n_best, n_add=n_add)


def test_large_skewed_problem():
    """2e7 calls, 2e5 barcodes, 64 donors, zipf coverage: 64-bit offsets, and positions with millions of calls."""
    rng = np.random.default_rng(7)
    calls = _random_calls(rng, 2, 20_000_000, 200_000, 100_000, skew=True)
    dob = rng.integers(-1, 64, 200_000).astype(np.int32)
    scored, selected = _device_run(_context(), calls, dob, 64, n_best=100, n_add=1000)
    assert scored['counts'].sum(axis=(1, 2)).max() > 1_000_000
    _check_against_restatement(scored, selected, calls, dob, 64, n_best=100, n_add=1000)


def test_detection_leaves_device_posteriors_and_state_alone():
    from demuxalot_amd import Demultiplexer
    from demuxalot_amd.device import DeviceContext
    fx, calls, genotypes, handler = r.load('f8_snp_synthetic.npz')
    posteriors = Demultiplexer.predict_posteriors(r.known_calls(calls, genotypes), genotypes, handler, doublet_prior=0.0,
                                                  on_device=True)
    try:
        best = posteriors.best()
        logits, probs = posteriors.to_dataframes()
        ctx = posteriors._ctx
        _sorted_donors, dob = r.donor_index(r.donor_map(fx), handler.ordered_barcodes)
        bytes_before = ctx.device_bytes()
        _device_run(ctx, calls, dob, len(_sorted_donors))
        after_best = posteriors.best()
        after_logits, after_probs = posteriors.to_dataframes()
        assert best.equals(after_best)
        fio.assert_bitwise(after_logits.values, logits.values, 'logits')
        fio.assert_bitwise(after_probs.values, probs.values, 'probs')
        assert ctx.device_bytes() > bytes_before
    finally:
        posteriors.close()
    # release_problem and destroy free the detection buffers
    fresh = DeviceContext(0)
    try:
        empty = fresh.device_bytes()
        _device_run(fresh, calls, dob, len(_sorted_donors))
        assert fresh.device_bytes() > empty
        fresh.release_problem()
        assert fresh.device_bytes() == empty
        with pytest.raises(Exception, match='call order'):
            fresh.snp_score(3.)
    finally:
        fresh.close()
