"""The pooled E-step with the grid of ambient fractions summed instead of searched (include/demux_hip_debug.h:
dmx_estep_ambient_grid_marginal; Demultiplexer.predict_posteriors_joint_ambient(over_grid='marginal')) restated with
numpy and the oracle, used as the checker by tests/test_ambient_marginal_cpu.py and tests/test_gpu_ambient_marginal.py.

S[b, k, j], the float64 sum of an option's log terms at grid point j, is recomputed here with np.bincount in call order
(tests/ambient_scoring_restatement.py keeps its sums to itself; tests/test_ambient_marginal_cpu.py pins f32(f64(pen) + S) to
tests/ambient_grid_restatement.py's profile bit for bit).  Then, per option row, j ascending, float32, every operation rounded:
    t = lambda[j] + lw[j]                                  a NaN is skipped
    first t:   jm = j; m = t; s = 1; u = alphas[j]
    t >  m:    r = exp(m - t); s = s r + 1; u = u r + alphas[j]; m = t; jm = j
    t == m:    s = s + 1; u = u + alphas[j]
    t <  m:    x = exp(t - m); s = s + x; u = u + alphas[j] x
    logit = f32( f64(pen) + (S[jm] + f64( f32(lw[jm] + log(s)) )) ),  alpha_mean = u / s
with exp and log the oracle's C restatements of numpy's float32 kernels (oracle/npsimd.c), sequential in j, vectorised over the rows.
The softmax and the read-outs go through oracle.softmax_rows, as tests/ambient_grid_restatement.restate builds them.  Nothing here knows
the library.

The second half holds the conditions the marginal has to meet on tests/ambient_grid_restatement.py's seeded simulation."""
import functools

import numpy as np

from oracle import demux_oracle
from tests import ambient_grid_restatement as grid_restated
from tests import ambient_restatement
from tests import ambient_scoring_restatement as scoring

DEFAULT_GRID = ambient_restatement.DEFAULT_GRID


def exp32(x):
    return demux_oracle._c_unary('npsimd_exp_array', np.asarray(x, dtype=np.float32))


def log32(x):
    return demux_oracle.log_f32(np.asarray(x, dtype=np.float32), impl='c')


def float64_sums(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, alphas, ambient):
    """(row_ptr int64[B + 1], S float64[row_ptr[B], A], pen float64[row_ptr[B]]): per option and grid point the float64 sum of
    f64(log(m keep + floor)) over the barcode's calls in stored order, and the option's penalty."""
    v, cb = np.asarray(v), np.asarray(cb)
    e = np.asarray(e, dtype=np.float32)
    prob = np.asarray(prob, dtype=np.float32)
    alphas = np.asarray(alphas, dtype=np.float32)
    ambient = np.asarray(ambient, dtype=np.float32)
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int64)
    pair_penalty = np.asarray(pair_penalty, dtype=np.float32)
    keep = 1 - e
    floor = e.clip(1e-4)
    assert keep.dtype == np.float32 and floor.dtype == np.float32
    widths = np.array([len(d) * (len(d) + 1) // 2 if with_doublets else len(d) for d in pools] + [0], dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(widths[pool_of_barcode])]).astype(np.int64)
    S = np.full((int(row_ptr[-1]), len(alphas)), np.nan, dtype=np.float64)
    pen = np.zeros(int(row_ptr[-1]), dtype=np.float64)
    for p, donors in enumerate(pools):
        rows = np.flatnonzero(pool_of_barcode == p)
        if not len(rows):
            continue
        mine = np.isin(cb, rows)  # (boolean selection keeps the stored order)
        vs, cbs, ks, fs = v[mine], cb[mine], keep[mine], floor[mine]
        d1, d2 = scoring.pool_options(donors, with_doublets)
        for k, (a, b) in enumerate(zip(d1, d2)):
            col = prob[:, a] if a == b else (prob[:, a] + prob[:, b]) * np.float32(0.5)
            own = col[vs]
            pen[row_ptr[rows] + k] = np.float64(0 if a == b else pair_penalty[p])
            for j, alpha in enumerate(alphas):
                m = own * (np.float32(1) - alpha) + ambient[vs] * alpha
                t = demux_oracle.log_f32(m * ks + fs)
                assert m.dtype == np.float32 and t.dtype == np.float32
                S[row_ptr[rows] + k, j] = np.bincount(cbs, weights=t, minlength=B)[rows]  # float64, in the order of the calls
    return row_ptr, S, pen


def over_the_grid(S, pen, alphas, log_weights=None):
    """The recurrence: (logits float32[n], alpha_index int32[n], alpha_mean float32[n], lam float32[n, A]) of the sums S[n, A]."""
    alphas = np.asarray(alphas, dtype=np.float32)
    n, A = S.shape
    lw = np.zeros(A, dtype=np.float32) if log_weights is None else np.asarray(log_weights, dtype=np.float32)
    assert lw.shape == (A,) and alphas.shape == (A,) and np.isfinite(lw).all()
    lam = (pen[:, None] + S).astype(np.float32)
    jm = np.full(n, -1, dtype=np.int32)
    m = np.full(n, np.nan, dtype=np.float32)
    s = np.ones(n, dtype=np.float32)
    u = np.zeros(n, dtype=np.float32)
    one = np.float32(1)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(A):
            t = lam[:, j] + lw[j]
            counts = ~np.isnan(t)
            first = counts & (jm < 0)
            above = counts & ~first & (t > m)
            equal = counts & ~first & (t == m)
            below = counts & ~first & (t < m)
            assert ((first | above | equal | below) == counts).all()
            r = exp32(np.where(above, m - t, np.float32(0)))
            x = exp32(np.where(below, t - m, np.float32(0)))
            s_above, u_above = s * r + one, u * r + alphas[j]
            s_equal, u_equal = s + one, u + alphas[j]
            s_below, u_below = s + x, u + alphas[j] * x
            s = np.where(first, one, np.where(above, s_above, np.where(equal, s_equal, np.where(below, s_below, s))))
            u = np.where(first, alphas[j], np.where(above, u_above, np.where(equal, u_equal, np.where(below, u_below, u))))
            assert s.dtype == np.float32 and u.dtype == np.float32 and t.dtype == np.float32
            moved = first | above
            m = np.where(moved, t, m)
            jm = np.where(moved, np.int32(j), jm)
    found = jm >= 0
    at = np.maximum(jm, 0)
    correction = lw[at] + log32(s)
    assert correction.dtype == np.float32
    with np.errstate(invalid='ignore'):
        total = pen + (S[np.arange(n), at] + correction.astype(np.float64))
        logits = np.where(found, total, np.nan).astype(np.float32)
        alpha_mean = np.where(found, u / s, np.float32(np.nan)).astype(np.float32)
    return logits, jm, alpha_mean, lam


def restate(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, alphas, ambient, log_weights=None):
    """dict(row_ptr, logits, probs, best_option, best_prob, doublet_mass, ambient, alpha_index, best_alpha_index, alpha_mean,
    best_alpha_mean, lam, S, pen) as dmx_estep_ambient_grid_marginal defines them."""
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int64)
    row_ptr, S, pen = float64_sums(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, alphas, ambient)
    logits, alpha_index, alpha_mean, lam = over_the_grid(S, pen, alphas, log_weights)
    probs = np.empty_like(logits)
    best_option = np.full(B, -1, dtype=np.int32)
    best_prob = np.full(B, np.nan, dtype=np.float32)
    doublet_mass = np.full(B, np.nan, dtype=np.float64)
    for p, donors in enumerate(pools):
        rows = np.flatnonzero(pool_of_barcode == p)
        if not len(rows):
            continue
        K = len(donors) * (len(donors) + 1) // 2 if with_doublets else len(donors)
        take = (row_ptr[rows][:, None] + np.arange(K, dtype=np.int64)[None, :]).reshape(-1)
        P = demux_oracle.softmax_rows(logits[take].reshape(len(rows), K))
        probs[take] = P.reshape(-1)
        masked = np.where(np.isnan(P), -np.inf, P)  # the first maximum; NaN never wins
        first = masked.argmax(axis=1)
        some = ~np.isnan(P).all(axis=1)
        best_option[rows] = np.where(some, first, -1)
        best_prob[rows] = np.where(some, P[np.arange(len(rows)), first], np.nan)
        pairs = P[:, len(donors):].astype(np.float64)  # added one after the other in ascending option order (cumsum is sequential)
        doublet_mass[rows] = np.cumsum(pairs, axis=1)[:, -1] if pairs.shape[1] else 0.0
    found = best_option >= 0
    best_alpha_index = np.full(B, -1, dtype=np.int32)
    best_alpha_index[found] = alpha_index[row_ptr[:-1][found] + best_option[found]]
    best_alpha_mean = np.full(B, np.nan, dtype=np.float32)
    best_alpha_mean[found] = alpha_mean[row_ptr[:-1][found] + best_option[found]]
    return dict(row_ptr=row_ptr, logits=logits, probs=probs, best_option=best_option, best_prob=best_prob, doublet_mass=doublet_mass,
                ambient=np.asarray(ambient, dtype=np.float32), alpha_index=alpha_index, best_alpha_index=best_alpha_index,
                alpha_mean=alpha_mean, best_alpha_mean=best_alpha_mean, lam=lam, S=S, pen=pen)


def restate_all_donors(v, cb, e, prob, B, doublet_prior, alphas, ambient, log_weights=None):
    """(logits, probs) [B, K] as predict_posteriors_joint_ambient(over_grid='marginal') returns them without pools, and the dict."""
    G = prob.shape[1]
    penalty = demux_oracle.doublet_penalties(G, doublet_prior)[-1] if G > 1 else 0.0
    out = restate(v, cb, e, prob, B, [list(range(G))], np.zeros(B, dtype=np.int32), np.array([penalty], dtype=np.float32), doublet_prior != 0,
                  alphas, ambient, log_weights)
    return out['logits'].reshape(B, -1), out['probs'].reshape(B, -1), out


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f'{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}'
    if got.tobytes() != want.tobytes():
        differ = np.flatnonzero(got.reshape(-1).view(f'u{got.itemsize}') != want.reshape(-1).view(f'u{want.itemsize}'))
        raise AssertionError(f'{what}: {len(differ)} of {got.size} differ, first at {differ[0]}: {got.reshape(-1)[differ[0]]!r} '
                             f'against {want.reshape(-1)[differ[0]]!r}')


SHARED = ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass')
OWN = ('alpha_index', 'best_alpha_index', 'alpha_mean', 'best_alpha_mean')


def assert_same(got, want, what):
    """Everything dmx_estep_ambient_grid_marginal returns, bit for bit (NaN payloads aside: a NaN is a NaN); `got` may lack the
    compact outputs that were not fetched."""
    for key in SHARED + OWN + ('ambient',):
        if got.get(key) is None:
            continue
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, f'{what}: {key}: {g.dtype}{g.shape} against {w.dtype}{w.shape}'
        if g.dtype.kind == 'f':
            assert np.array_equal(np.isnan(g), np.isnan(w)), f'{what}: {key}: NaN in other places'
            keep = ~np.isnan(w)
            same_bits(g[keep], w[keep], f'{what}: {key}')
        else:
            assert np.array_equal(g, w), f'{what}: {key}'


# ---- the simulation's conditions --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def simulated(calls_per_barcode, seed=0, doublet_prior=0.35):
    """(sim, the max mode restated, the marginal restated): tests/ambient_grid_restatement.simulated's problem - default grid, derived
    profile - under both modes.  Computed once per shape, shared."""
    sim = grid_restated.simulate(seed, calls_per_barcode)
    soup = ambient_restatement.derived_ambient(sim['v'], sim['v2snp'], 0.01)
    _l, _p, marginal = restate_all_donors(sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B'], doublet_prior, DEFAULT_GRID, soup)
    # the max mode from the same sums: the first maximum of lambda, one softmax (ambient_grid_restatement.restate's construction)
    index, logits = ambient_restatement.first_maximum(marginal['lam'])
    K = marginal['lam'].shape[0] // sim['B']
    P = demux_oracle.softmax_rows(logits.reshape(sim['B'], K))
    G = sim['prob'].shape[1]
    best = np.where(np.isnan(P), -np.inf, P).argmax(axis=1).astype(np.int32)
    maximum = dict(logits=logits, probs=P.reshape(-1), best_option=best, alpha_index=index,
                   doublet_mass=np.cumsum(P[:, G:].astype(np.float64), axis=1)[:, -1],
                   best_alpha_index=index.reshape(sim['B'], K)[np.arange(sim['B']), best])
    return sim, maximum, marginal


def counts_of(sim, doublet_mass, best_option):
    """dict(doublets_called, singlets_called_doublets, singlets_right): "doublet" is pair mass above 0.5."""
    counts = grid_restated.joint_counts(sim, doublet_mass, best_option, np.zeros(sim['B']))
    return {key: counts[key] for key in ('doublets_called', 'singlets_called_doublets', 'singlets_right')}


def marginal_conditions(calls_per_barcode, sim, max_counts, counts):
    """The conditions on seed 0, default grid, derived profile, doublet_prior 0.35 - conditions with slack, not measurements.
    64 calls: at least 30 of 48 true doublets called doublets, at least 5 more than the max mode in the same run, at most 7 of 96
    singlets called doublets, at least 89 singlets right.  256 calls: at least 42 doublets called, at most 2 singlets called doublets,
    at least 94 singlets right."""
    assert sim['B'] == 144 and int((sim['second'] < 0).sum()) == 96
    print(f'{calls_per_barcode} calls per barcode: max {max_counts}, marginal {counts}')
    if calls_per_barcode == 64:
        assert counts['doublets_called'] >= 30, counts
        assert counts['doublets_called'] >= max_counts['doublets_called'] + 5, (max_counts, counts)
        assert counts['singlets_called_doublets'] <= 7, counts
        assert counts['singlets_right'] >= 89, counts
    elif calls_per_barcode == 256:
        assert counts['doublets_called'] >= 42, counts
        assert counts['singlets_called_doublets'] <= 2, counts
        assert counts['singlets_right'] >= 94, counts
    else:
        raise AssertionError('no conditions for this shape')
    return counts
