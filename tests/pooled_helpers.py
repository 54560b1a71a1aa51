"""What the GPU tests of the pooled entries share (tests/test_gpu_pools*.py, _ambient*, _pair_shares, _doublet*_learning): the names
of the fixtures, the comparisons that judge a result, how a fixture or a designed problem gets onto a context, the designed problems
themselves, the step-wise learning loop and the refusals every pooled entry owes its pool arguments.  tests/test_pooled_helpers_cpu.py
shows that the comparisons still bite and pins the designed problems' bytes.

The module imports without a GPU: a DeviceContext is only made inside the functions that need one.  A context is never shared between
test modules - the tests change its mode and its additions - so every module keeps the contexts it made in a cache of its own:
    resident = functools.lru_cache(maxsize=None)(pooled_helpers.new_resident)"""
import os

import numpy as np
import pytest

from tests import ambient_restatement
from tests import fixture_io as fio
from tests import pools_learning_restatement
from tests import pools_restatement

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = -1, -5
F1, F2 = 'f1_synthetic_default.npz', 'f2_synthetic_g4.npz'  # G = 20, B = 1000; G = 4
F3_SMALL = ['f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz']  # (f3_small_2.npz: G = 5)
WIDE = 'f3_small_4.npz'  # G = 70, B = 24
POOLS_F1 = [list(range(8)), list(range(4, 12)), [0, 19], [3, 7, 11, 15, 18], list(range(5, 18)), [19]]  # overlapping; donor 18 alone in none


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
def same_bytes(got, want, keys, what):
    """The two results hold the same bytes under every key: the same type, the same bits (-0 is not 0, one NaN not another)."""
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), f'{what}: {key}'


def assert_iteration(ctx, got, want, what, addition=None, same=pools_restatement.assert_same):
    """One E-step's results against a record of the restatement; the dense matrix is the context's resident posteriors, and where the
    E-step returns a soup profile that is compared too.  `same` judges the E-step's own outputs."""
    same(got, want, what)
    fio.assert_bitwise(ctx.get_probs(), want['dense'], f'{what}: get_probs()')
    if 'ambient' in got:
        fio.assert_bitwise(got['ambient'], want['ambient'], f'{what}: the soup profile')
    if addition is not None:
        fio.assert_bitwise(addition, want['addition'], f'{what}: addition')


def at(array, index, value):
    """A copy of the array with one entry changed."""
    out = np.array(array, copy=True)
    out[index] = value
    return out


# ---- a fixture or a designed problem on a context ---------------------------------------------------------------------------------
def new_resident(name, clip=0.01, extra_barcodes=0):
    """(ctx, v, cb, e, prob, B, v2snp): a fixture's packed problem and its genotype table resident on a new context;
    extra_barcodes: that many barcodes without any call behind the fixture's."""
    from demuxalot_amd.device import DeviceContext
    fx = fio.load(name)
    v, cb, e, prob, B, v2snp = ambient_restatement.fixture_problem(name, clip)
    B += extra_barcodes
    ctx = DeviceContext(0)
    ctx.set_problem(B, len(v2snp), prob.shape[1], v, cb, e, v2snp)
    ctx.set_betas(fx['pack0_betas'])
    ctx.set_addition(None)
    fio.assert_bitwise(ctx.probs_from_betas(clip), prob, f'{name}: genotype table')
    return ctx, v, cb, e, prob, B, v2snp


def install(ctx, name):
    """The fixture's packed problem and its prior betas (raw betas + the data prior: learn_genotypes's own) on a context."""
    fx = fio.load(name)
    problem = pools_learning_restatement.fixture_learning_problem(name)
    V, G = problem['betas'].shape
    ctx.set_problem(problem['B'], V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
    molecules = np.bincount(problem['v'], weights=fx['pack_bc_variant_count'], minlength=V).astype(np.int64)
    betas = ctx.set_prior_betas(problem['raw_betas'], float(fx['default_prior']), True, mol_per_variant=molecules)
    fio.assert_bitwise(betas, problem['betas'], f'{name}: prior betas')
    return ctx


def new_learner(name):
    """A new context with the fixture installed for learning."""
    from demuxalot_amd.device import DeviceContext
    return install(DeviceContext(0), name)


def install_designed(ctx, problem):
    """A problem given as a dict (v, cb, e, v2snp, betas, B) on a context, its betas as they are."""
    V, G = problem['betas'].shape
    ctx.set_problem(problem['B'], V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
    ctx.set_betas(problem['betas'])
    return ctx


# ---- problem builders -------------------------------------------------------------------------------------------------------------
def pool_of_f1(B=1000):
    """The pool of every barcode of f1 among POOLS_F1: every seventh barcode in none."""
    pool_of = (np.arange(B) * 5) % 7
    return np.where(pool_of == 6, -1, pool_of).astype(np.int32)


def pools_of(name, B, G):
    """(pools, pool_of): the overlapping pools on f1, one all-donor pool on every other fixture."""
    return (POOLS_F1, pool_of_f1()) if name == F1 else ([list(range(G))], np.zeros(B, np.int32))


def pair_penalty(pools, dp):
    """What the Python layer passes: the reference's bonus for a list of g_p genotypes, 0 for a single donor or without doublets."""
    penalties = pools_restatement.demux_oracle.doublet_penalties
    return np.array([penalties(len(d), dp)[-1] if len(d) > 1 and dp != 0 else 0.0 for d in pools], dtype=np.float32)


def spread_columns(rng, n, G=1024):
    """n of the table's G columns, ascending, drawn all over the table."""
    return sorted(int(d) for d in rng.choice(G, size=n, replace=False))


def designed_grid(n, seed_base=100):
    """n grid values: unsorted, with both ends 1 and 0 (from two values on) and duplicated values (from three on; the 0 twice, so that a
    barcode without calls, and every other tie, has to take the lower index)."""
    values = np.random.default_rng(seed_base + n).uniform(0, 1, size=n).astype(np.float32)
    if n >= 2:
        values[0], values[-1] = 1.0, 0.0
    if n >= 3:
        values[1] = 0.0
    if n >= 8:
        values[n // 2], values[n - 3] = values[3], values[2]
    return values


def designed_arrays(lengths, V, B, seed, zero_share=None):
    """(v, cb, e, prob, v2snp, soup, lengths) of a designed problem: B barcodes, barcode i with lengths[i % len(lengths)] calls, on 1024
    donors and V / 2 biallelic SNPs; error probabilities at both ends of their range among them, the ends of the range in the table's
    first row and in the soup, and with zero_share that share of the table's entries exactly 0.  The problems sit on kernel edges (slot
    boundaries, the 8-call padding): the random draws are taken in this order and no other, and tests/test_pooled_helpers_cpu.py pins
    the bytes."""
    rng = np.random.default_rng(seed)
    G = 1024
    lengths = [lengths[i % len(lengths)] for i in range(B)]
    v2snp = np.repeat(np.arange(V // 2, dtype=np.int32), 2)
    v = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for n in lengths]).astype(np.int32)
    cb = np.repeat(np.arange(B), lengths).astype(np.int32)
    e = rng.choice(np.array([0.0, 1e-5, 1e-4, 0.01, 0.3, 1.0], dtype=np.float32), size=len(v))
    order = np.lexsort((cb, v))
    v, cb, e = v[order], cb[order], e[order]
    prob = rng.uniform(0.01, 0.99, size=(V, G)).astype(np.float32)
    if zero_share is not None:
        prob[rng.random(size=prob.shape) < zero_share] = 0.0  # entries of exactly 0 ...
    prob[0, :3] = [0.0, 1.0, 0.5]  # ... and the other end (row 0 is what the padding calls point at)
    soup = rng.uniform(0, 1, size=V).astype(np.float32)
    soup[:3] = [1.0, 0.0, 0.5]
    assert np.bincount(cb, minlength=B).tolist() == lengths
    return v, cb, e, prob, v2snp, soup, np.asarray(lengths)


def install_arrays(v, cb, e, prob, v2snp, soup, lengths):
    """(ctx, v, cb, e, prob, B, v2snp, soup, lengths): designed_arrays' problem and its table on a new context."""
    from demuxalot_amd.device import DeviceContext
    V, G = prob.shape
    ctx = DeviceContext(0)
    ctx.set_problem(len(lengths), V, G, v, cb, e, v2snp)
    ctx.set_probs(prob)
    return ctx, v, cb, e, prob, len(lengths), v2snp, soup, lengths


def user_inputs(sim, betas, default_prior):
    """(calls, genotypes, handler): a simulated problem as a user holds it - one molecule per call on one chromosome, the reference
    allele 'A' and the alternative 'C' at position s + 1 of SNP s, genotypes with the given betas and default prior."""
    from demuxalot_amd import BarcodeHandler, CompressedSNPCalls, ProbabilisticGenotypes
    n = len(sim['v'])
    calls = {'chr1': CompressedSNPCalls.from_arrays(sim['cb'], np.arange(n), sim['v'] // 2 + 1, sim['v'] % 2, sim['e'])}
    genotypes = ProbabilisticGenotypes([f'donor{g}' for g in range(sim['prob'].shape[1])], default_prior=default_prior)
    genotypes.var2varid = {('chr1', int(row) // 2 + 1, 'AC'[int(row) % 2]): int(row) for row in range(len(sim['v2snp']))}
    genotypes.variant_betas = np.array(betas, copy=True)
    handler = BarcodeHandler([f'BC{b:03d}-1' for b in range(sim['B'])])
    assert handler.ordered_barcodes == [f'BC{b:03d}-1' for b in range(sim['B'])]
    return calls, genotypes, handler


def table_betas(sim):
    """Betas that are the simulation's allele probabilities times 1000: what user_inputs takes with default prior 1."""
    return (sim['prob'] * np.float32(1000)).astype(np.float32)


# ---- the step-wise learning loop, and the exact mode ------------------------------------------------------------------------------
def staged(ctx, n, clip, estep, mstep):
    """The step-wise path: per iteration (E-step results, the addition its table was made with).  estep() runs the module's resident
    E-step, mstep(its results) the M-step behind it and returns the addition."""
    ctx.set_addition(None)
    addition = np.zeros((ctx.V, ctx.G), np.float32)
    for it in range(n):
        ctx.probs_from_betas(clip, fetch=False)
        out = estep()
        yield out, addition
        if it + 1 < n:
            addition = mstep(out)


@pytest.fixture
def exact_mode():
    """The default context's passes in the exact arithmetic: what a new pass is compared with bit for bit.  A module that uses the
    fixture imports it by name."""
    from demuxalot_amd.device import get_context
    previous = os.environ.get('DEMUXALOT_AMD_ESTEP')
    os.environ['DEMUXALOT_AMD_ESTEP'] = 'exact'
    get_context().apply_environment()
    try:
        yield
    finally:
        if previous is None:
            os.environ.pop('DEMUXALOT_AMD_ESTEP', None)
        else:
            os.environ['DEMUXALOT_AMD_ESTEP'] = previous
        get_context().apply_environment()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def pool_refusal_cases(good, pool_of):
    """The eight (change, code, message) every pooled entry owes its pool arguments, as changes of `good`: a raw call of the pools
    [[0, 1], [1, 2, 4]] of five donors with doublets.  A module puts them in front of its own cases."""
    assert list(good['pool_start']) == [0, 2, 5] and list(good['donors']) == [0, 1, 1, 2, 4] and good['with_doublets'] == 1
    bad_rows = np.array(good['row_ptr'], copy=True)
    bad_rows[1:] += 1
    return [
        (dict(pool_start=[1, 2, 5]), DMX_ERR_INVALID, 'pool_start[0]'),
        (dict(pool_start=[0, 2, 2, 5], penalty=[0, 0, 0]), DMX_ERR_INVALID, 'empty'),
        (dict(donors=[0, 1, 2, 1, 4]), DMX_ERR_INVALID, 'ascending'),
        (dict(donors=[0, 1, 1, 2, 5]), DMX_ERR_INVALID, 'outside'),
        (dict(pool_of=at(pool_of, 1, 2)), DMX_ERR_INVALID, 'pool_of_barcode'),
        (dict(row_ptr=bad_rows), DMX_ERR_INVALID, 'row_ptr'),
        (dict(with_doublets=2), DMX_ERR_INVALID, 'with_doublets'),
        (dict(n_pools=-1), DMX_ERR_INVALID, 'n_pools'),
    ]


def check_needs_problem_table_no_communicator(raw_call, entry_name, args):
    """An entry refuses a context without a problem, one without a table and one with a communicator, names itself and writes nothing;
    with a problem and a table it runs.  raw_call(ctx, **args) -> (status, message, whether an output was written), args for the
    problem of f3_small_0.npz."""
    from demuxalot_amd.device import DeviceContext
    v, cb, e, prob, B, v2snp = ambient_restatement.fixture_problem('f3_small_0.npz')
    V, G = prob.shape
    with DeviceContext(0) as ctx:
        status, text, written = raw_call(ctx, **args)
        assert status == DMX_ERR_INVALID and 'call order' in text and entry_name in text and not written
        ctx.set_problem(B, V, G, v, cb, e, v2snp)
        status, text, written = raw_call(ctx, **args)
        assert status == DMX_ERR_INVALID and 'call order' in text and not written
        ctx.set_probs(prob)
        status, _text, written = raw_call(ctx, **args)
        assert status == 0 and written
    with DeviceContext(0) as ctx:
        ctx.comm_init_emulated(0, 1)
        ctx.set_problem(B, V, G, v, cb, e, v2snp)
        ctx.set_probs(prob)
        status, text, written = raw_call(ctx, **args)
        assert status == DMX_ERR_UNSUPPORTED and 'communicator' in text and entry_name in text and not written
