"""What tests/test_gpu_aggregate_shapes.py relies on, checked without a GPU: the numpy restatement of the float64 M-step is the
reference's (bit for bit on the F7 fixtures' own posteriors), the designed problems of tests/aggregate_problems.py hold what their
docstrings say, every case runs the kernel form its id names, and no barcode's oracle posteriors are near a tie."""
import numpy as np
import pytest

from tests import aggregate_problems as ap
from tests import fixture_io as fio

F7 = ['f7_aggregate_small_2.npz', 'f7_aggregate_small_4.npz', 'f7_aggregate_synthetic_g4.npz', 'f7_aggregate_synthetic_default.npz']
ALL_CASES = sorted(set(ap.ESTEP_CASES + ap.PRIOR_CASES + ap.MSTEP_CASES) | {(5, True, 'wave1')}, key=lambda c: (c[1], c[0]))


@pytest.mark.parametrize('name', F7)
def test_restated_mstep_is_the_reference_s_on_its_own_posteriors(oracle, name):
    """em{i}_it{t + 1}_addition of every F7 run is, bit for bit, mstep_f64_restated of em{i}_it{t}_probs - the reference's captured
    float64 posteriors - on the packed barcode calls."""
    out = fio.load(name)
    fx = fio.load(str(out['inputs_of']))
    packed = oracle.pack(fio.oracle_calls(fx), fio.oracle_geno(fx), add_data_prior=True)
    V, G = packed['betas'].shape
    compared = 0
    for i in range(int(out['n_em'])):
        for it in range(int(out[f'em{i}_n_iterations']) - 1):
            post = out[f'em{i}_it{it}_probs']
            assert post.dtype == np.float64
            got = ap.mstep_f64_restated(packed['variant_id'], packed['compressed_cb'], packed['p_base_wrong'], post, V, G, 2.)
            fio.assert_bitwise(got, out[f'em{i}_it{it + 1}_addition'], f'{name} run {i} addition after iteration {it}')
            sums = ap.mstep_f64_restated(packed['variant_id'], packed['compressed_cb'], packed['p_base_wrong'], post, V, G, 2., as_float64=True)
            assert sums.dtype == np.float64
            fio.assert_bitwise(sums.astype(np.float32), got, 'the unrounded sums round to the addition')
            compared += 1
    assert compared > 0


def _pair_ids(problem):
    """Per molecule call: the (barcode, SNP) pair as one integer."""
    return problem['mcb'].astype(np.int64) * ap.N_SNPS + problem['v2snp'][problem['mv']]


@pytest.mark.parametrize('G', [1, 2, 3, 65, 1025])
def test_shape_problem_holds_what_it_claims(G):
    p = ap.shape_problem(G)
    assert p['B'] == 9 and p['B'] % 4 != 0 and p['V'] == 2 * ap.N_SNPS and p['prob'].shape == (p['V'], G) and p['prob'].dtype == np.float32
    per_barcode = np.bincount(p['mcb'], minlength=p['B'])
    assert list(per_barcode) == [0, 1, ap.LONG_COUNT + 11, sum(range(2, 8)), 6, 5, 33, 65, 0]
    # the barcodes are interleaved in molecule order: nothing is grouped before the device groups it
    assert (np.diff(p['mcb']) < 0).sum() > 50
    # the table: uniform without plateaus but for the designed zeros
    zero = np.argwhere(p['prob'] == 0)
    assert [tuple(z) for z in zero] == [(2 * ap.ZERO_SNP, g) for g in ap.zeroed_columns(G)]
    positive = p['prob'][p['prob'] > 0]
    assert positive.min() > 0.02 and positive.max() < 0.98
    # barcode 2: one pair of 300 calls on both variants of its SNP, eleven pairs of one
    pairs = _pair_ids(p)
    ids, counts = np.unique(pairs[p['mcb'] == 2], return_counts=True)
    assert sorted(counts) == [1] * 11 + [ap.LONG_COUNT] and ids[counts.argmax()] == 2 * ap.N_SNPS + ap.LONG_SNP
    assert set(p['mv'][pairs == 2 * ap.N_SNPS + ap.LONG_SNP]) == {2 * ap.LONG_SNP, 2 * ap.LONG_SNP + 1}
    assert np.unique(pairs, return_counts=True)[1].max() == ap.LONG_COUNT
    # barcode 3: inside every pair the variants alternate in molecule order, and the pairs' calls are interleaved
    mine = np.flatnonzero(p['mcb'] == 3)
    ids = np.unique(pairs[mine])
    assert len(ids) == 6
    assert sorted(np.unique(pairs[mine], return_counts=True)[1]) == [2, 3, 4, 5, 6, 7]
    for pair in ids:
        variants = p['mv'][mine[pairs[mine] == pair]]
        assert (np.diff(variants) != 0).all() and set(variants) == {variants[0], variants[0] ^ 1}
    assert (np.diff(pairs[mine]) != 0).sum() > 15
    # barcode 4: p + e == 0 at the designed options of one pair, and only there
    hit = np.flatnonzero((p['mcb'] == 4) & (p['mv'] == 2 * ap.ZERO_SNP))
    assert len(hit) == 1 and p['mp'][hit[0]] == 0 and (p['mp'][np.arange(len(p['mp'])) != hit[0]] > 0).all()
    assert ((p['mcb'] == 4) & (p['mv'] == 2 * ap.ZERO_SNP + 1)).sum() == 1
    assert len(ap.options_at_minus_inf(G, False)) == min(2, G - 1) and len(ap.options_at_minus_inf(G, True)) == (3 if G >= 3 else G - 1)
    # barcodes 5 .. 7: repeated pairs
    for b in ap.OTHERS:
        assert np.unique(pairs[p['mcb'] == b], return_counts=True)[1].max() > 1 or b == 5
    assert np.unique(pairs[p['mcb'] == 7], return_counts=True)[1].max() > 2
    # barcode calls: distinct, shuffled, for every barcode; the last SNP has none of either kind
    assert len(np.unique(np.stack([p['v'], p['cb']]), axis=1).T) == len(p['v'])
    assert set(p['cb']) == set(range(9)) and (np.diff(p['v']) < 0).any()
    assert p['v'].max() < p['V'] - 2 and p['mv'].max() < p['V'] - 2
    assert p['e'].dtype == np.float32 and p['mp'].dtype == np.float32


@pytest.mark.parametrize('G, doublets', [(3, False), (3, True), (65, False), (11, True)])
def test_options_at_minus_inf_are_finite_in_the_oracle_s_output(oracle, G, doublets):
    """The -inf terms of barcode 4: in float32, p + e is 0 at exactly the designed options of the designed call, and the oracle's
    logits and posteriors are finite everywhere, the empty barcodes' +0 and 1 / K."""
    p = ap.shape_problem(G)
    g1, g2 = oracle.option_pairs(G, 0.5 if doublets else 0.)
    K = ap.n_options(G, doublets)
    assert len(g1) == K
    table = np.where(g1 == g2, p['prob'][:, g1], (p['prob'][:, g1] + p['prob'][:, g2]) * np.float32(0.5))
    terms = table[p['mv']] + p['mp'][:, None]
    assert terms.dtype == np.float32
    calls, options = np.nonzero(terms == 0)
    assert set(calls) == {int(np.flatnonzero((p['mcb'] == 4) & (p['mv'] == 2 * ap.ZERO_SNP))[0])}
    assert sorted(options) == sorted(ap.options_at_minus_inf(G, doublets)) and 0 < len(options) < K
    logits, probs = ap.expected(oracle, p, doublets)
    assert logits.shape == (p['B'], K) and np.isfinite(logits).all() and np.isfinite(probs).all()
    for b in (0, p['B'] - 1):
        assert (logits[b] == 0).all() and not np.signbit(logits[b]).any() and (probs[b] == 1 / K).all()


def test_oracle_handles_no_molecule_calls_at_all(oracle):
    p = ap.shape_problem(5)
    nothing = dict(p, mv=p['mv'][:0], mcb=p['mcb'][:0], mp=p['mp'][:0])
    logits, probs = ap.expected(oracle, nothing, True)
    assert logits.shape == (9, 15) and (logits == 0).all() and not np.signbit(logits).any() and (probs == 1 / 15).all()


def test_item_problem_holds_what_it_claims():
    p = ap.item_problem()
    per_variant = np.bincount(p['v'], minlength=p['V'])
    assert p['prob'].shape[1] == 65 and p['hot'] == 0
    assert per_variant[p['hot']] == ap.ITEM_HOT_CALLS > 2 * ap.ITEM_CALLS and per_variant[p['hot']] <= 3 * ap.ITEM_CALLS
    assert (per_variant[p['uncalled']] == 0).all() and (per_variant[np.setdiff1d(np.arange(p['V']), p['uncalled'])] > 0).all()
    assert len(p['v']) <= 6000 * ap.ITEM_CALLS  # so few calls are cut into items of 1024: csrc/kernels.h, item_calls_for
    assert len(np.unique(np.stack([p['v'], p['cb']]), axis=1).T) == len(p['v'])
    assert 1.0e6 < p['B'] * 65 * 8 < 1.2e6
    assert not (np.diff(p['cb'][p['v'] == p['hot']]) > 0).all()  # the hot variant's calls are not in barcode order


@pytest.mark.parametrize('case', ALL_CASES, ids=ap.case_id)
def test_every_case_runs_the_form_its_id_names(case):
    G, doublets, form = case
    K = ap.n_options(G, doublets)
    if form.startswith('m'):
        assert ap.mstep_form(G) == form
        assert ap.estep_form(K) is not None
    else:
        assert ap.estep_form(K) == form


def test_the_cases_lie_on_both_sides_of_every_boundary():
    for doublets in (True, False):
        forms = [ap.estep_form(ap.n_options(G, doublets)) for G, d, _ in ap.ESTEP_CASES if d == doublets]
        Gs = [G for G, d, _ in ap.ESTEP_CASES if d == doublets]
        for G, form in zip(Gs, forms):  # every case is the first or the last G of its form (G = 1 and the widest table apart)
            first = G == 1 or ap.estep_form(ap.n_options(G - 1, doublets)) != form
            last = ap.estep_form(ap.n_options(G + 1, doublets)) != form
            assert first or last, (G, doublets, form)
    assert {form for _, _, form in ap.ESTEP_CASES} == {f'wave{A}' for A in (1, 2, 4, 8, 16)} | {f'block{A}' for A in (6, 9, 12, 17, 24, 33)}
    assert {(form, d) for _, d, form in ap.ESTEP_CASES} >= {(f'wave{A}', d) for A in (1, 2, 4, 8, 16) for d in (True, False)} | {('block6', False)}
    assert {ap.mstep_form(G) for G, _, _ in ap.MSTEP_CASES} == {'m1', 'm2', 'm4', 'm8', 'm16', 'm16x2'}
    for G, doublets in ap.REFUSED_CASES:
        assert ap.estep_form(ap.n_options(G, doublets)) is None and ap.estep_form(ap.n_options(G - 1, doublets)) == 'block33'


@pytest.mark.parametrize('case', ALL_CASES, ids=ap.case_id)
def test_no_barcode_with_calls_is_near_a_tie(oracle, case):
    """The arg-max assertion of the GPU tests means something: on every barcode with molecule calls the oracle's two largest
    posteriors are at least 1e-9 apart (the device's are within 1e-12).  No barcode is left out."""
    G, doublets, _ = case
    p = ap.shape_problem(G)
    _, probs = ap.expected(oracle, p, doublets)
    if probs.shape[1] == 1:
        return  # one option: nothing to tie with
    top = np.sort(probs, axis=1)[:, -2:]
    with_calls = np.bincount(p['mcb'], minlength=p['B']) > 0
    assert with_calls.sum() == 7
    assert (top[with_calls, 1] - top[with_calls, 0]).min() >= 1e-9, (top[:, 1] - top[:, 0])


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['prior32', 'prior64'])
@pytest.mark.parametrize('case', ap.PRIOR_CASES, ids=ap.case_id)
def test_no_barcode_is_near_a_tie_under_the_prior(oracle, case, dtype):
    """With the prior of the GPU test added, on every barcode - those without calls take the prior itself."""
    G, doublets, _ = case
    prior = ap.prior_logits(G, doublets, dtype)
    assert prior.dtype == dtype and not np.signbit(prior[prior == 0]).any()
    probs = ap.softmax64(ap.expected(oracle, ap.shape_problem(G), doublets)[0] + prior)
    top = np.sort(probs, axis=1)[:, -2:]
    assert (top[:, 1] - top[:, 0]).min() >= 1e-9


def test_no_barcode_of_the_item_problem_is_near_a_tie(oracle):
    p = ap.item_problem()
    _, probs = ap.expected(oracle, p, False)
    top = np.sort(probs, axis=1)[:, -2:]
    assert (np.bincount(p['mcb'], minlength=p['B']) > 0).all()
    assert (top[:, 1] - top[:, 0]).min() >= 1e-9
