"""Demultiplexer.aggregate_on_snps = True (demux.py:204-244) on the GPU against the reference's captured outputs
(F7 fixtures: tests/golden/make_fixtures.py: aggregate_on_snps_cases).

Everything up to the first log_softmax is float32 arithmetic reproduced bit for bit (numpy's float32 log / exp /
pairwise sums, float64 accumulation in molecule order); np.logaddexp and the second log_softmax are float64, where
numpy's exp / log / log1p are its own SIMD kernels or libm depending on the host CPU and the device has the ROCm
device library's.  The gate is therefore: assignments identical, posteriors within 1e-12 (the contract says 1e-5),
logits within 1e-11 relative; the achieved agreement in float64 ulps is printed."""
import numpy as np
import pytest

from tests import fixture_io as fio

pytestmark = pytest.mark.gpu

NAMES = ['f7_aggregate_small_2.npz', 'f7_aggregate_small_4.npz', 'f7_aggregate_synthetic_g4.npz',
         'f7_aggregate_synthetic_default.npz']


@pytest.fixture()
def aggregating():
    from demuxalot_amd import Demultiplexer
    Demultiplexer.aggregate_on_snps = True
    yield Demultiplexer
    Demultiplexer.aggregate_on_snps = False


def check64(got_logits, got_probs, ref_logits, ref_probs, what):
    assert got_logits.dtype == np.float64 and got_probs.dtype == np.float64, what
    assert np.array_equal(got_probs.argmax(axis=1), ref_probs.argmax(axis=1)), f'{what}: assignments differ'
    assert np.abs(got_probs - ref_probs).max() <= 1e-12, f'{what}: posteriors {np.abs(got_probs - ref_probs).max():.3g}'
    assert np.allclose(got_logits, ref_logits, rtol=1e-11, atol=1e-11), f'{what}: logits {np.abs(got_logits - ref_logits).max():.3g}'
    return float((np.abs(got_logits - ref_logits) / np.spacing(np.abs(ref_logits))).max())


@pytest.mark.parametrize('name', NAMES)
def test_aggregate_on_snps_matches_reference(aggregating, name):
    D = aggregating
    out = fio.load(name)
    fx = fio.load(str(out['inputs_of']))
    calls, genotypes, handler = fio.product_inputs(fx)
    worst = 0.0
    for i in range(int(out['n_predict'])):
        logits_df, probs_df = D.predict_posteriors(calls, genotypes, handler, doublet_prior=float(out[f'predict{i}_dp']))
        assert logits_df.index.name == 'BARCODE' and list(logits_df.columns) == [str(c) for c in out[f'predict{i}_columns']]
        worst = max(worst, check64(logits_df.values, probs_df.values, out[f'predict{i}_logits'], out[f'predict{i}_probs'],
                                   f'{name} predict {i}'))
    for i in range(int(out['n_em'])):
        kwargs = dict(n_iterations=int(out[f'em{i}_n_iterations']), doublet_prior=float(out[f'em{i}_dp']))
        prior = out.get(f'em{i}_prior_logits')
        stages = list(D.staged_genotype_learning(calls, genotypes, handler,
                                                 barcode_prior_logits=None if prior is None else prior.copy(), **kwargs))
        for it, (probs_df, dbg) in enumerate(stages):
            worst = max(worst, check64(dbg['barcode_logits'], probs_df.values, out[f'em{i}_it{it}_logits'],
                                       out[f'em{i}_it{it}_probs'], f'{name} run {i} it {it}'))
            want = out[f'em{i}_it{it}_addition']
            assert dbg['genotype_addition'].dtype == np.float32
            assert np.allclose(dbg['genotype_addition'], want, rtol=3e-7, atol=0), f'{name} run {i} it {it} addition'
            assert (dbg['genotype_addition'] != want).mean() <= 1e-3  # a float64 ulp upstream rarely moves a float32 rounding
        learnt, last = D.learn_genotypes(calls, genotypes, handler,
                                         barcode_prior_logits=None if prior is None else prior.copy(), **kwargs)
        assert np.allclose(learnt.variant_betas, out[f'em{i}_learnt_betas'], rtol=3e-7, atol=0)
        assert np.array_equal(last.values, stages[-1][0].values)
    print(f'{name}: float64 logits within {worst:.1f} ulp of the reference')


def test_aggregate_dispatcher_on_caller_supplied_tables(aggregating, oracle):
    """compute_barcode_logits with molecule_calls (the dispatcher of demux.py:193-202) against the oracle."""
    D = aggregating
    fx = fio.load('f3_small_3.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    v2snp, betas, molecule_calls, barcode_calls = D.pack_calls(calls, genotypes, add_data_prior=False)
    prob = oracle.probs_from_betas(v2snp, betas, 0.01)
    for dp in (0., 0.3):
        want = oracle.barcode_logits_aggregated(molecule_calls['variant_id'], molecule_calls['compressed_cb'],
                                                molecule_calls['p_base_wrong'], v2snp, prob, handler.n_barcodes, dp)
        got, names = D.compute_barcode_logits(genotypes.genotype_names, barcode_calls, molecule_calls, dp, prob,
                                              handler.n_barcodes, genotypes.n_genotypes)
        assert got.dtype == np.float64 and len(names) == want.shape[1]
        assert np.allclose(got, want, rtol=1e-11, atol=1e-11)


def test_aggregate_mode_refuses_what_it_cannot_do(aggregating):
    fx = fio.load('f3_small_0.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    with pytest.raises(AssertionError, match='float64'):
        aggregating.predict_posteriors(calls, genotypes, handler, on_device=True)


@pytest.mark.parametrize('n_genotypes', [60, 75, 100, 128])
def test_aggregate_wide_option_tables_against_the_oracle(oracle, n_genotypes):
    """Doublets of 60 / 75 / 100 / 128 genotypes (1830 / 2850 / 5050 / 8256 options: the workgroup-per-barcode kernel
    with 9 / 12 / 24 / 33 options per thread) on synthetic molecule calls with repeated (barcode, SNP) pairs."""
    from demuxalot_amd import synth
    from demuxalot_amd.device import get_context
    p = synth.generate(40, 300, n_genotypes, calls_per_barcode=60, seed=n_genotypes)
    rng = np.random.default_rng(n_genotypes)
    # molecule calls: every barcode call 1..3 times, in shuffled (molecule) order
    rep = rng.integers(1, 4, size=len(p.variant_id))
    order = rng.permutation(int(rep.sum()))
    mv, mcb = np.repeat(p.variant_id, rep)[order], np.repeat(p.compressed_cb, rep)[order]
    mp = rng.uniform(0.001, 0.2, size=len(mv)).astype(np.float32)
    ctx = get_context()
    ctx.set_problem(p.n_barcodes, p.n_variants, n_genotypes, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
    ctx.set_betas(p.prior_betas())
    ctx.set_addition(None)
    prob = ctx.probs_from_betas(0.01)
    ctx.set_molecule_calls(mv, mcb, mp)
    logits, probs = ctx.estep_snp(True, 0.5)
    want = oracle.barcode_logits_aggregated(mv, mcb, mp, p.v2snp, prob, p.n_barcodes, 0.5)
    assert logits.shape == want.shape == (40, n_genotypes * (n_genotypes + 1) // 2)
    assert np.allclose(logits, want, rtol=1e-11, atol=1e-11), np.abs(logits - want).max()
    shifted = np.exp(want - want.max(axis=1, keepdims=True))  # scipy softmax, float64
    want_probs = shifted / shifted.sum(axis=1, keepdims=True)
    assert np.array_equal(probs.argmax(axis=1), want_probs.argmax(axis=1)) and np.abs(probs - want_probs).max() <= 1e-12
    print(f'G={n_genotypes}: float64 logits within {(np.abs(logits - want) / np.spacing(np.abs(want))).max():.1f} ulp of the oracle')


def test_float32_and_float64_e_steps_with_different_option_counts_on_one_context():
    """Call order through the raw entry points: a float32 E-step with singlets (K = G), then an aggregate E-step with
    doublets (K = G (G + 1) / 2) on the same context and back.  Results laid out for the other option count must read
    as absent (an error), never as out-of-bounds device reads."""
    from demuxalot_amd import Demultiplexer, synth
    from demuxalot_amd._lib import DemuxHipError
    from demuxalot_amd.device import DeviceContext
    p = synth.generate(300, 200, 5, calls_per_barcode=30, seed=9)
    G = 5
    ctx = DeviceContext(0)
    try:
        ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        ctx.set_molecule_calls(p.variant_id, p.compressed_cb, p.p_base_wrong)
        ctx.set_betas(p.prior_betas())
        ctx.set_addition(None)
        ctx.probs_from_betas(0.01, fetch=False)
        logits32, probs32 = ctx.estep(Demultiplexer._doublet_penalties(G, 0.), with_doublets=False)
        assert probs32.shape == (300, 5)
        logits64, probs64 = ctx.estep_snp(True, 0.5)  # K = 15 now
        assert probs64.shape == (300, 15)
        with pytest.raises(DemuxHipError):  # the float32 posteriors belong to K = 5
            ctx.get_probs()
        with pytest.raises(DemuxHipError):
            ctx.mstep(2.)
        add64 = ctx.mstep_f64(2.)
        assert add64.shape == (p.n_variants, G) and np.isfinite(add64).all()
        from tests.aggregate_problems import mstep_f64_restated  # the M-step is deterministic given the device's own posteriors
        fio.assert_bitwise(add64, mstep_f64_restated(np.asarray(p.variant_id), np.asarray(p.compressed_cb), np.asarray(p.p_base_wrong, dtype=np.float32),
                                                     probs64, p.n_variants, G, 2.), 'float64 M-step after E-steps of two option counts')
        logits32b, probs32b = ctx.estep(Demultiplexer._doublet_penalties(G, 0.), with_doublets=False)  # K = 5 again
        fio.assert_bitwise(probs32b, probs32, 'float32 E-step repeated after the aggregate one')
        with pytest.raises(DemuxHipError):  # the float64 posteriors belong to K = 15
            ctx.mstep_f64(2.)
        assert np.isfinite(ctx.mstep(2.)).all()
    finally:
        ctx.close()
