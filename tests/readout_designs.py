"""Designed posteriors for the read-out tests (tests/test_readout_designs_cpu.py, tests/test_gpu_readout_shapes.py).

A flat E-step - a genotype table that is 0.5 everywhere and the same single call for every barcode - gives every option of a barcode
the same evidence, so the logits of a row are `penalties + prior_logits[b]` up to that common term and the posteriors their softmax:
equal inputs give bit-equal posteriors, and a logit of -200 gives an exact float32 zero (exp underflows).  The designs below place
a handful of chosen logits in chosen columns and -200 everywhere else.  Nothing here is an expectation of a read-out: the tests take
their references from the posteriors the device holds, and use structure() only to assert that those posteriors have the designed
edge (the ties, the zeros, the all-NaN row) before they check anything.

The first half is pure numpy; install() puts a design on a DeviceContext."""
import numpy as np

ZERO_LOGIT = np.float32(-200.0)  # softmax gives an exact float32 zero next to any logit of the designs (all within [-5, 0])
WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 256, 257, 320, 321, 2080, 8256)
BARCODES = (1, 4, 5, 37)  # a workgroup of the wavefront-per-barcode kernels takes four barcodes
P_BASE_WRONG = np.float32(0.1)


def shape_for(K):
    """(G, with_doublets) with K options.  Singlet tables up to 1024 genotypes have an E-step (csrc/estep_plan.h: kernel());
    2080 and 8256 are the pairs of 64 and 128 donors, 3 those of 2."""
    pairs = {3: 2, 2080: 64, 8256: 128}
    if K in pairs:
        G = pairs[K]
        assert G * (G + 1) // 2 == K
        return G, True
    assert 1 <= K <= 1024
    return K, False


def barcode_counts(K):
    """The widest table runs with at most five barcodes (the restatements walk every column in Python)."""
    return BARCODES if K < 8256 else BARCODES[:3]


def _descending(columns):
    return {c: -float(j) for j, c in enumerate(columns)}


def placement(name, K):
    """{column: logit} of the named placement at width K - every other column gets ZERO_LOGIT - or None where K has no room for it.
    'flat' is the whole row equal (returned as an empty dict with background 0)."""
    if name == 'flat':
        return {}
    if name.startswith('one_lane_'):  # the five largest values in lane l: columns l, l + 64, ..., l + 256 (as many as K holds)
        _, _, order, lane = name.split('_')
        columns = [c for c in range(int(lane[1:]), K, 64)][:5]
        if len(columns) < 2:
            return None
        # a lane meets its columns in ascending order: 'asc' has the largest value arrive last, 'desc' first
        return _descending(columns if order == 'desc' else columns[::-1])
    if name == 'edges':  # the last column, lane 0 and lane 63 hold the largest values
        columns = list(dict.fromkeys(c for c in (K - 1, 0, 63) if c < K))
        return _descending(columns) if len(columns) >= 2 else None
    if name in ('tie_63_64', 'tie_0_64', 'tie_1_64', 'tie_1_64_second'):  # a tied pair, first or (under column 5) second
        if K < 65:
            return None
        a, b = (int(x) for x in name.split('_')[1:3])
        second = name.endswith('_second')
        values = {a: -1.0 if second else 0.0, b: -1.0 if second else 0.0, 5: 0.0 if second else -1.0}
        for j, c in enumerate(range(69, min(K, 262), 64)):  # 69, 133, 197, 261: lane 5 again, descending
            values[c] = -2.0 - j
        return values
    if name == 'tie3_lane2':  # three equal values inside one lane
        return {2: 0.0, 66: 0.0, 130: 0.0, 3: -1.0} if K >= 131 else None
    if name == 'tie_4th_5th':
        if K >= 65:  # the tied pair: the lower column sits in the higher lane
            return {7: 0.0, (70 if K > 70 else 20): -1.0, 30: -2.0, 1: -3.0, 64: -3.0}
        return {K - 1: 0.0, K - 2: -1.0, K - 3: -2.0, 0: -3.0, 1: -3.0} if K >= 5 else None
    if name == 'two_nonzero':  # the 3rd and 4th places go to the lowest zero columns
        if K < 2:
            return None
        return {K - 1: 0.0, (K // 2 if K // 2 != K - 1 else 0): -1.0}
    raise KeyError(name)


PLACEMENTS = ('flat', 'one_lane_asc_l0', 'one_lane_asc_l5', 'one_lane_asc_l63', 'one_lane_desc_l0', 'one_lane_desc_l5',
              'one_lane_desc_l63', 'edges', 'tie_63_64', 'tie_0_64', 'tie_1_64', 'tie_1_64_second', 'tie3_lane2', 'tie_4th_5th',
              'two_nonzero')


def catalogue():
    """[(K, name, B)]: every placement at every width that has room for it; the barcode counts go round within a width, and the
    flat row runs at each of them."""
    cases = []
    for K in WIDTHS:
        counts = barcode_counts(K)
        names = [name for name in PLACEMENTS if placement(name, K) is not None]
        for i, name in enumerate(names):
            cases.append((K, name, counts[i % len(counts)]))
        cases += [(K, 'flat', B) for B in counts[1:]]
    return cases


def design_row(name, K):
    """float32[K]: the designed logits of the unrotated row."""
    values = placement(name, K)
    assert values is not None, (name, K)
    row = np.full(K, 0.0 if name == 'flat' else ZERO_LOGIT, dtype=np.float32)
    for column, value in values.items():
        row[column] = value
    return row


def shifts(K, B):
    """Row b carries the design rotated by 17 b columns: the rows differ and the best column moves across lanes."""
    return (np.arange(B) * 17) % K


def designed_logits(name, K, B):
    """float32[B, K]: what `penalties + prior_logits` is meant to be, row by row."""
    row = design_row(name, K)
    return np.stack([np.roll(row, int(s)) for s in shifts(K, B)]) if B else np.zeros((0, K), np.float32)


def design(name, K, B):
    """(G, with_doublets, penalties float32[K], prior_logits float32[B, K] or None).  One barcode: the design is the penalties,
    no prior.  More: the prior carries the rotated rows and the penalties are zero, so that equal designed logits are equal
    (penalty, prior) pairs and stay bit-equal through the float32 additions of the E-step."""
    G, with_doublets = shape_for(K)
    if B == 1:
        return G, with_doublets, design_row(name, K), None
    return G, with_doublets, np.zeros(K, dtype=np.float32), designed_logits(name, K, B)


def nan_design(K, B, row, column):
    """The rotated 'two_nonzero' rows (K >= 2) with one NaN in the prior of `row`: that row has no non-NaN posterior."""
    G, with_doublets = shape_for(K)
    prior = designed_logits('two_nonzero', K, B)
    prior[row, column] = np.nan
    return G, with_doublets, np.zeros(K, dtype=np.float32), prior


def random_design(K, B, seed=0):
    """Random priors (posteriors over several orders of magnitude, no structure): for the sums, the masses and the blocks."""
    G, with_doublets = shape_for(K)
    rng = np.random.default_rng([seed, K, B])
    return G, with_doublets, np.zeros(K, dtype=np.float32), (3 * rng.standard_normal((B, K))).astype(np.float32)


def intended_top(name, K, k=4):
    """The columns the unrotated row is meant to rank first: designed values descending, ties and the zeros by column."""
    values = placement(name, K)
    ranked = sorted(values, key=lambda c: (-values[c], c))
    return (ranked + [c for c in range(K) if c not in values])[:k]


def structure(P, L, what=''):
    """Asserts that the float32 posteriors P have the structure of the designed logits L, row by row: bit-equal where the logits
    are equal, strictly ordered where they differ, exact zeros at ZERO_LOGIT (and nowhere else), all NaN in a row whose logits
    hold a NaN.  A test calls this before it checks anything, so that it cannot pass on a matrix that lacks its edge."""
    P, L = np.asarray(P), np.asarray(L)
    assert P.dtype == np.float32 and P.shape == L.shape, (what, P.dtype, P.shape, L.shape)
    for r in range(len(P)):
        if np.isnan(L[r]).any():
            assert np.isnan(P[r]).all(), f'{what}: row {r} has a NaN logit, its posteriors are not all NaN: {P[r][:8]}'
            continue
        assert np.isfinite(P[r]).all(), f'{what}: row {r} is not finite'
        zero = L[r] == ZERO_LOGIT
        assert (P[r][zero] == 0).all() and (P[r][~zero] > 0).all(), \
            f'{what}: row {r} has {int((P[r] == 0).sum())} exact zeros, designed {int(zero.sum())}'
        order = np.argsort(L[r], kind='stable')
        ls, ps = L[r][order], P[r][order].view(np.uint32).astype(np.int64)  # (non-negative floats order like their bits)
        equal = ls[1:] == ls[:-1]
        assert (ps[1:][equal] == ps[:-1][equal]).all(), f'{what}: row {r}: equal logits, posteriors that differ in their bits'
        assert (ps[1:][~equal] > ps[:-1][~equal]).all(), f'{what}: row {r}: ordered logits, posteriors that are not'


def flat_evidence_posteriors(oracle, G, with_doublets, penalties, prior_logits, B):
    """The oracle's E-step (oracle/demux_oracle.py: barcode_logits, em, softmax_rows) on the flat problem install() sets up, with
    these penalties in the place of the doublet penalties: float32 logits = penalty + the float64 sum of a barcode's one
    float32 log term, then the prior, then the float32 softmax."""
    K = G * (G + 1) // 2 if with_doublets else G
    keep, floor = 1 - P_BASE_WRONG, np.maximum(P_BASE_WRONG, np.float32(1e-4))
    term = oracle.log_f32(np.full(B, 0.5, dtype=np.float32) * keep + floor)  # pairs: (0.5 + 0.5) * 0.5, the same
    logits = np.zeros([B, 1], dtype='float32') + np.asarray(penalties, dtype=np.float32)
    for k in range(K):
        logits[:, k] = logits[:, k] + np.bincount(np.arange(B), weights=term, minlength=B)
    if prior_logits is not None:
        logits += prior_logits
    with np.errstate(invalid='ignore'):
        return oracle.softmax_rows(logits)


def install(G, with_doublets, penalties, prior_logits, B):
    """A DeviceContext holding the flat problem - B barcodes with one call each of the same variant, a table of 0.5 - one exact
    E-step with these penalties and priors behind it.  The caller closes it."""
    from demuxalot_amd.device import DeviceContext
    ctx = DeviceContext(0)
    try:
        ctx.set_estep_mode('exact')  # the subject is the read-outs, not the guard
        ctx.set_problem(B, 2, G, np.zeros(B, dtype=np.int32), np.arange(B, dtype=np.int32), np.full(B, P_BASE_WRONG, dtype=np.float32),
                        np.zeros(2, dtype=np.int32))
        ctx.set_probs(np.full((2, G), 0.5, dtype=np.float32))
        ctx.estep(penalties, with_doublets=with_doublets, prior_logits=prior_logits, fetch_logits=False, fetch_probs=False)
    except BaseException:
        ctx.close()
        raise
    return ctx
