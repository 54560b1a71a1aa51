"""The device pack (csrc/repack_device.hip: variant table, compaction, stable radix sort, products in input order,
molecule counts, the container paths) on the problems of tests/pack_problems.py, against the oracle: through every entry
point, into the data prior, into an E-step on the layouts derived from the device-resident unique calls, into the kept
molecule calls of aggregate_on_snps, and through the refusals.  tests/test_pack_fuzz_cpu.py shows on the CPU that the
table holds the edges it is there for and that the host twin agrees with the same expected values.

Integers are compared with array_equal, float32 bit for bit; the float64 logits of the aggregate E-step with the
tolerance of tests/test_gpu_aggregate.py."""
import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pack_problems as pp

pytestmark = pytest.mark.gpu

G = pp.G
SMALL = [name for name, case in pp.CASES.items() if case['V'] <= 1025]


@pytest.fixture()
def ctx():
    from demuxalot_amd.device import DeviceContext
    context = DeviceContext(0)
    try:
        yield context
    finally:
        context.close()


def keys_of(prob):
    return prob.var_chrom, prob.var_pos, prob.var_base, prob.v2snp


def pack_flat(ctx, prob):
    return ctx.pack_and_set_problem(prob.n_barcodes, G, *keys_of(prob), prob.chrom, prob.pos, prob.base, prob.cb, prob.p)


def pack_containers(ctx, prob):
    return ctx.pack_containers_and_set_problem(prob.n_barcodes, G, *keys_of(prob), pp.container_list(prob))


def pack_staged(ctx, prob, table=None):
    ctx.stage_containers(pp.container_list(prob, provisional=True))
    return ctx.pack_staged_and_set_problem(prob.n_barcodes, G, *keys_of(prob), pp.chrom_of_container(prob) if table is None else table)


ENTRY_POINTS = {'flat': pack_flat, 'containers': pack_containers, 'staged': pack_staged}


def packed(ctx, answer):
    n_matched, n_unique, mol = answer
    return (n_matched, n_unique, mol) + tuple(ctx.get_packed_calls())


def assert_packed(got, want, what):
    n_matched, n_unique, mol, variant, cb, p, count = got
    assert (n_matched, n_unique) == (want.n_matched, want.n_unique), what
    assert mol.dtype == np.int64 and np.array_equal(mol, want.mol_per_variant), what
    assert np.array_equal(variant, want.variant) and np.array_equal(cb, want.cb) and np.array_equal(count, want.count), what
    fio.assert_bitwise(p, want.p, f'{what}: p_base_wrong products')


def random_betas(prob, seed):
    rng = np.random.default_rng(seed)
    betas = (rng.gamma(0.5, 30.0, size=(prob.n_variants, G)) + 0.01).astype(np.float32)
    return rng, betas


@pytest.mark.parametrize('name', list(pp.CASES))
def test_entry_points_agree_with_the_oracle(ctx, oracle, name):
    prob, want = pp.problem(name), pp.expected_of(name, oracle)
    got = {}
    for entry, pack in ENTRY_POINTS.items():
        got[entry] = packed(ctx, pack(ctx, prob))
        assert_packed(got[entry], want, f'{name} through {entry}')
    for entry in ('containers', 'staged'):
        for a, b in zip(got[entry], got['flat']):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f'{name}: {entry} against flat'


@pytest.mark.parametrize('name', list(pp.CASES))
def test_data_prior_uses_the_counts_the_pack_left(ctx, oracle, name):
    prob, want = pp.problem(name), pp.expected_of(name, oracle)
    pack_staged(ctx, prob)
    rng, raw = random_betas(prob, 11)
    raw[rng.random(raw.shape) < 0.1] = 0
    assert len(np.unique(prob.v2snp)) < prob.n_variants or prob.n_variants < 6, 'SNPs with several variants'
    got = ctx.set_prior_betas(raw, 1.0, True, mol_per_variant=None)
    fio.assert_bitwise(got, oracle.prior_betas(raw, prob.v2snp, want.mol_variant, 1.0, True), f'{name}: prior betas with the data prior')


@pytest.mark.parametrize('name', SMALL)
def test_estep_on_the_layouts_of_the_packed_problem(ctx, oracle, name):
    from demuxalot_amd import Demultiplexer
    prob, want = pp.problem(name), pp.expected_of(name, oracle)
    pack_flat(ctx, prob)
    _rng, betas = random_betas(prob, 12)
    ctx.set_betas(betas)
    ctx.set_addition(None)
    prob_table = oracle.probs_from_betas(prob.v2snp, betas, 0.01)
    fio.assert_bitwise(ctx.probs_from_betas(0.01), prob_table, f'{name}: genotype probabilities')
    logits, _probs = ctx.estep(Demultiplexer._doublet_penalties(G, 0.), with_doublets=False)
    fio.assert_bitwise(logits, oracle.barcode_logits(want.variant, want.cb, want.p, prob_table, prob.n_barcodes, 0., log_impl='npsimd'),
                       f'{name}: logits of the packed problem')


@pytest.mark.parametrize('name,entry', [('long_v1023', 'flat'), ('edges_v1025', 'staged')])
def test_kept_molecule_calls(ctx, oracle, name, entry):
    """aggregate_on_snps reads the matched molecule calls the pack keeps: the long runs, and a chromosome split over two
    containers.  Tolerance of tests/test_gpu_aggregate.py."""
    prob, want = pp.problem(name), pp.expected_of(name, oracle)
    ctx.set_keep_molecule_calls(True)
    assert_packed(packed(ctx, ENTRY_POINTS[entry](ctx, prob)), want, name)
    _rng, betas = random_betas(prob, 13)
    ctx.set_betas(betas)
    ctx.set_addition(None)
    prob_table = ctx.probs_from_betas(0.01)
    logits, _probs = ctx.estep_snp(True, 0.5)
    ref = oracle.barcode_logits_aggregated(want.mol_variant, want.mol_cb, want.mol_p, prob.v2snp, prob_table, prob.n_barcodes, 0.5)
    assert logits.shape == ref.shape == (prob.n_barcodes, G * (G + 1) // 2)
    print(f'{name}: float64 logits within {np.abs(logits - ref).max():.3g} of the oracle')
    assert np.allclose(logits, ref, rtol=1e-11, atol=1e-11), np.abs(logits - ref).max()


# ---- refusals: every one answers a status before a kernel indexes with the bad value, and the context packs on -------------
REFUSALS = 'n512'


def a_call(want, matched, k=3):
    return int(np.flatnonzero((want.call_variant >= 0) == matched)[k])


@pytest.mark.parametrize('entry', list(ENTRY_POINTS))
def test_negative_barcode_on_a_matched_call_is_refused(ctx, oracle, entry):
    from demuxalot_amd._lib import DemuxHipError
    prob, want = pp.problem(REFUSALS), pp.expected_of(REFUSALS, oracle)
    with pytest.raises(DemuxHipError, match=r'negative barcode.*status -1\)'):
        ENTRY_POINTS[entry](ctx, pp.with_barcode(prob, a_call(want, True), -1))
    assert_packed(packed(ctx, ENTRY_POINTS[entry](ctx, prob)), want, f'{entry} after the refusal')


@pytest.mark.parametrize('entry', list(ENTRY_POINTS))
def test_negative_barcode_on_an_unmatched_call_goes_with_the_call(ctx, oracle, entry):
    """As the host twin does (pack_host.cpp: the barcode is looked at after the match)."""
    prob, want = pp.problem(REFUSALS), pp.expected_of(REFUSALS, oracle)
    assert_packed(packed(ctx, ENTRY_POINTS[entry](ctx, pp.with_barcode(prob, a_call(want, False), -1))), want, entry)
    assert_packed(packed(ctx, ENTRY_POINTS[entry](ctx, prob)), want, f'{entry}, the plain problem next')


@pytest.mark.parametrize('entry', list(ENTRY_POINTS))
def test_barcode_beyond_the_last_is_refused(ctx, oracle, entry):
    from demuxalot_amd._lib import DemuxHipError
    prob, want = pp.problem(REFUSALS), pp.expected_of(REFUSALS, oracle)
    with pytest.raises(DemuxHipError, match=rf'compressed_cb\[\d+\]={prob.n_barcodes} outside \[0,{prob.n_barcodes}\).*status -1\)'):
        ENTRY_POINTS[entry](ctx, pp.with_barcode(prob, a_call(want, True), prob.n_barcodes))
    assert_packed(packed(ctx, ENTRY_POINTS[entry](ctx, prob)), want, f'{entry} after the refusal')


def test_staged_calls_without_a_chromosome_and_pack_without_a_staging_are_refused(ctx, oracle):
    from demuxalot_amd._lib import DemuxHipError
    prob, want = pp.problem(REFUSALS), pp.expected_of(REFUSALS, oracle)
    table = pp.chrom_of_container(prob)
    filled = next(k for k, (_chrom, c) in enumerate(prob.containers) if c.n_snp_calls)
    with pytest.raises(DemuxHipError, match=r'calls on a chromosome without variants.*status -1\)'):
        pack_staged(ctx, prob, table[:filled] + [-1] + table[filled + 1:])
    with pytest.raises(DemuxHipError, match=r'call order.*status -1\)'):   # the refusal released the staging
        ctx.pack_staged_and_set_problem(prob.n_barcodes, G, *keys_of(prob), table)
    assert_packed(packed(ctx, pack_staged(ctx, prob)), want, 'staged after the refusals')
    with pytest.raises(DemuxHipError, match=r'call order.*status -1\)'):   # a staging is used once
        ctx.pack_staged_and_set_problem(prob.n_barcodes, G, *keys_of(prob), table)
    assert_packed(packed(ctx, pack_flat(ctx, prob)), want, 'flat after the refusals')


@pytest.mark.parametrize('entry', list(ENTRY_POINTS))
def test_no_variants_or_no_calls_is_an_empty_problem(ctx, oracle, entry):
    """V = 0 with calls and n = 0 with variants are no errors (csrc/dmx_api.cpp checks the sizes for < 0 only): nothing
    matches, and the resident problem has no calls."""
    import copy
    prob, want = pp.problem(REFUSALS), pp.expected_of(REFUSALS, oracle)
    no_variants = copy.copy(prob)
    no_variants.var_chrom, no_variants.var_pos, no_variants.v2snp = (np.zeros(0, dtype=np.int32) for _ in range(3))
    no_variants.var_base, no_variants.n_variants = np.zeros(0, dtype=np.uint8), 0
    no_calls = pp.problem('n0')
    for what, empty in (('V = 0', no_variants), ('n = 0', no_calls)):
        n_matched, n_unique, mol, variant, cb, p, count = packed(ctx, ENTRY_POINTS[entry](ctx, empty))
        assert (n_matched, n_unique) == (0, 0), what
        assert mol.shape == (empty.n_variants,) and not mol.any(), what
        assert len(variant) == len(cb) == len(p) == len(count) == 0, what
    assert_packed(packed(ctx, ENTRY_POINTS[entry](ctx, prob)), want, f'{entry} after the empty problems')
