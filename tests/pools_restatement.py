"""The pooled E-step (include/demux_hip_debug.h: dmx_estep_pools; Demultiplexer.predict_posteriors_in_pools) restated with the oracle,
used as the checker by tests/test_pools_cpu.py and tests/test_gpu_pools.py.

The row of a barcode of pool p is row b of what the reference computes for the genotype list d_p on the column subset of the same
table: oracle.barcode_logits(v, cb, e, prob[:, d_p], B, doublet_prior) followed by oracle.softmax_rows.  So for every distinct donor
list the oracle runs once on prob[:, d_p], over all barcodes, and the rows of the pool's barcodes are cut out; row_ptr, the compact
rows, the first arg-max and the float64 pair mass (ascending option order) are built in numpy.  Nothing here knows the library."""
import numpy as np

from oracle import demux_oracle
from tests import fixture_io as fio


def fixture_problem(name, clip=0.01):
    """(v, cb, e, prob, B) of a golden fixture as predict_posteriors sees it (prior betas without the data term)."""
    fx = fio.load(name)
    prob = demux_oracle.probs_from_betas(fx['pack_v2snp'], fx['pack0_betas'], clip)
    return fx['pack_bc_variant_id'], fx['pack_bc_cb'], fx['pack_bc_p'], prob, len(fx['barcodes'])


class Restatement:
    """The oracle's full-B result per distinct donor list of one problem, computed once and kept (the tests share it)."""

    def __init__(self, v, cb, e, prob, B, doublet_prior):
        self.v, self.cb, self.e, self.prob, self.B, self.doublet_prior = v, cb, e, np.asarray(prob, dtype=np.float32), B, doublet_prior
        self._of_donors = {}

    def pool_rows(self, donors):
        """(logits, probs) [B, K_p] of the genotype list `donors` (ascending table columns)."""
        key = tuple(int(d) for d in donors)
        assert list(key) == sorted(set(key)) and len(key) >= 1, 'a pool is a strictly ascending list of columns'
        if key not in self._of_donors:
            logits = demux_oracle.barcode_logits(self.v, self.cb, self.e, self.prob[:, list(key)], self.B, self.doublet_prior)
            self._of_donors[key] = (logits, demux_oracle.softmax_rows(logits))
        return self._of_donors[key]

    def pair_penalty(self, pools):
        """What the Python layer passes: the reference's bonus for a list of g_p genotypes, 0 for a single donor."""
        return np.array([demux_oracle.doublet_penalties(len(d), self.doublet_prior)[-1] if len(d) > 1 else 0.0 for d in pools],
                        dtype=np.float32)

    def __call__(self, pools, pool_of_barcode):
        """dict(row_ptr, logits, probs, best_option, best_prob, doublet_mass) as dmx_estep_pools defines them."""
        pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
        assert pool_of_barcode.shape == (self.B,)
        widths = np.array([len(d) * (len(d) + 1) // 2 if self.doublet_prior != 0 else len(d) for d in pools] + [0], dtype=np.int64)
        row_ptr = np.concatenate([[0], np.cumsum(widths[pool_of_barcode])]).astype(np.int64)
        logits = np.empty(int(row_ptr[-1]), dtype=np.float32)
        probs = np.empty(int(row_ptr[-1]), dtype=np.float32)
        best_option = np.full(self.B, -1, dtype=np.int32)
        best_prob = np.full(self.B, np.nan, dtype=np.float32)
        doublet_mass = np.full(self.B, np.nan, dtype=np.float64)
        for p, donors in enumerate(pools):
            rows = np.flatnonzero(pool_of_barcode == p)
            if not len(rows):
                continue
            L, P = (m[rows] for m in self.pool_rows(donors))
            K = L.shape[1]
            take = (row_ptr[rows][:, None] + np.arange(K, dtype=np.int64)[None, :]).reshape(-1)
            logits[take] = L.reshape(-1)
            probs[take] = P.reshape(-1)
            # the first maximum; NaN never wins (a row of NaNs: -1 / NaN)
            masked = np.where(np.isnan(P), -np.inf, P)
            first = masked.argmax(axis=1)
            some = ~np.isnan(P).all(axis=1)
            best_option[rows] = np.where(some, first, -1)
            best_prob[rows] = np.where(some, P[np.arange(len(rows)), first], np.nan)
            # the pair posteriors widened to float64 and added one after the other in ascending option order (cumsum is sequential)
            pairs = P[:, len(donors):].astype(np.float64)
            doublet_mass[rows] = np.cumsum(pairs, axis=1)[:, -1] if pairs.shape[1] else 0.0
        return dict(row_ptr=row_ptr, logits=logits, probs=probs, best_option=best_option, best_prob=best_prob, doublet_mass=doublet_mass)


def assert_same(got, want, what):
    """Everything bit for bit (NaN read-outs of barcodes in no pool: NaN on both sides)."""
    assert np.array_equal(got['row_ptr'], want['row_ptr']), what
    fio.assert_bitwise(got['logits'], want['logits'], f'{what}: logits')
    fio.assert_bitwise(got['probs'], want['probs'], f'{what}: probs')
    assert got['best_option'].dtype == np.int32 and np.array_equal(got['best_option'], want['best_option']), f'{what}: best_option'
    none = want['best_option'] < 0
    assert np.isnan(got['best_prob'][none]).all() and np.isnan(got['doublet_mass'][none]).all(), f'{what}: NaN where there is no option'
    fio.assert_bitwise(got['best_prob'][~none], want['best_prob'][~none], f'{what}: best_prob')
    assert got['doublet_mass'].dtype == np.float64
    fio.assert_bitwise(got['doublet_mass'][~none], want['doublet_mass'][~none], f'{what}: doublet_mass')
