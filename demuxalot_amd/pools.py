"""Posteriors within per-barcode donor pools (Demultiplexer.predict_posteriors_in_pools).

A pool is a lane, hashtag group or sub-experiment that holds a known subset of the donors of one genotype table.  Each barcode
is scored against the donors of its own pool only, so its row has the pool's options - the singlets of the pool's donors in
genotype order, then their pairs - and the rows of different pools have different lengths.  The result is therefore COMPACT: one
flat float32 array per matrix and a row pointer, host-resident.  Per pool it unfolds into the DataFrames the reference returns for
that genotype sub-list.
"""
import numpy as np
import pandas as pd


def resolve_pools(genotype_names, ordered_barcodes, barcode2pool, pool2donors):
    """(pool names, per pool the ascending table columns of its donors, pool_of_barcode int32[B] with -1 for 'in no pool').
    Donor names are accepted in any order and sorted into genotype order, so that a pool's columns are the reference's for that
    genotype list.  ValueError: an empty pool, a duplicate or unknown donor name, a barcode that is missing from barcode2pool, an
    unknown pool name."""
    column_of = {name: i for i, name in enumerate(genotype_names)}
    pool_names, pool_columns = [], []
    for pool, donors in pool2donors.items():
        donors = list(donors)
        if not donors:
            raise ValueError(f'pool {pool!r} has no donors')
        unknown = [d for d in donors if d not in column_of]
        if unknown:
            raise ValueError(f'pool {pool!r}: unknown donor(s) {unknown!r}')
        if len(set(donors)) != len(donors):
            raise ValueError(f'pool {pool!r} lists a donor more than once')
        pool_names.append(pool)
        pool_columns.append(sorted(column_of[d] for d in donors))
    index_of = {pool: i for i, pool in enumerate(pool_names)}
    pool_of_barcode = np.empty(len(ordered_barcodes), dtype=np.int32)
    for b, barcode in enumerate(ordered_barcodes):
        if barcode not in barcode2pool:
            raise ValueError(f'barcode {barcode!r} is missing from barcode2pool (None says: in no pool)')
        pool = barcode2pool[barcode]
        if pool is None:
            pool_of_barcode[b] = -1
        elif pool in index_of:
            pool_of_barcode[b] = index_of[pool]
        else:
            raise ValueError(f'barcode {barcode!r}: unknown pool {pool!r}')
    return pool_names, pool_columns, pool_of_barcode


class PooledPosteriors:
    """Logits and posteriors of one predict_posteriors_in_pools call, compact and host-resident.

    pool_names / pool_columns: per pool its name and the names of its options; pool_of_barcode int32[B] (-1: in no pool);
    row_ptr int64[B + 1]: barcode b owns logits[row_ptr[b]:row_ptr[b + 1]] and the same entries of probs; best_option,
    best_prob, doublet_mass: the per-barcode read-outs of the pass (-1 / NaN / NaN for a barcode in no pool)."""

    def __init__(self, barcodes, pool_names, pool_columns, pool_of_barcode, row_ptr, logits, probs, best_option, best_prob,
                 doublet_mass, index_name='BARCODE'):
        self.barcodes = list(barcodes)
        self._pool_names = list(pool_names)
        self._pool_columns = [list(c) for c in pool_columns]
        self.pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.logits = np.asarray(logits, dtype=np.float32)
        self.probs = np.asarray(probs, dtype=np.float32)
        self.best_option = np.asarray(best_option, dtype=np.int32)
        self.best_prob = np.asarray(best_prob, dtype=np.float32)
        self.doublet_mass = np.asarray(doublet_mass, dtype=np.float64)
        self.index_name = index_name
        B = len(self.barcodes)
        assert len(self._pool_names) == len(self._pool_columns)
        assert self.pool_of_barcode.shape == (B,) and self.row_ptr.shape == (B + 1,)
        assert self.best_option.shape == (B,) and self.best_prob.shape == (B,) and self.doublet_mass.shape == (B,)
        assert self.logits.shape == self.probs.shape == (int(self.row_ptr[-1]) if B else 0,)
        widths = np.array([len(c) for c in self._pool_columns] + [0], dtype=np.int64)  # (-1 -> no entries)
        assert np.array_equal(np.diff(self.row_ptr), widths[self.pool_of_barcode]), 'row_ptr does not follow the pools'

    @property
    def pools(self):
        return list(self._pool_names)

    def _index(self, barcodes):
        index = pd.Index(barcodes)
        index.name = self.index_name
        return index

    def _pool_index(self, pool):
        if pool not in self._pool_names:
            raise KeyError(f'unknown pool {pool!r}')
        return self._pool_names.index(pool)

    def columns_of(self, pool):
        """The option names of a pool: its donors in genotype order, then 'A+B' for A before B."""
        return list(self._pool_columns[self._pool_index(pool)])

    def barcodes_of(self, pool):
        """The pool's barcodes, in handler order."""
        rows = np.flatnonzero(self.pool_of_barcode == self._pool_index(pool))
        return [self.barcodes[i] for i in rows]

    def to_dataframes(self, pool):
        """(logits_df, probs_df) of one pool: what the reference's predict_posteriors returns for the pool's genotype sub-list,
        restricted to the pool's barcodes (handler order)."""
        p = self._pool_index(pool)
        columns = self._pool_columns[p]
        rows = np.flatnonzero(self.pool_of_barcode == p)
        take = (self.row_ptr[rows][:, None] + np.arange(len(columns), dtype=np.int64)[None, :]).reshape(-1)
        shape = (len(rows), len(columns))
        barcodes = [self.barcodes[i] for i in rows]
        return (pd.DataFrame(self.logits[take].reshape(shape), index=self._index(barcodes), columns=columns),
                pd.DataFrame(self.probs[take].reshape(shape), index=self._index(barcodes), columns=columns))

    def best(self) -> pd.DataFrame:
        """Per barcode (all of them, handler order): its pool, the most probable option of the pool and its posterior; None /
        None / NaN for a barcode in no pool."""
        pool = np.asarray(self._pool_names + [None], dtype=object)[self.pool_of_barcode]
        option = np.empty(len(self.barcodes), dtype=object)
        for b, (p, k) in enumerate(zip(self.pool_of_barcode, self.best_option)):
            option[b] = self._pool_columns[p][k] if p >= 0 and k >= 0 else None
        return pd.DataFrame({'pool': pool, 'option': option, 'probability': self.best_prob}, index=self._index(self.barcodes))

    def assignments(self, threshold=0.9) -> pd.Series:
        """probs[probs.max(axis=1).gt(threshold)].idxmax(axis=1) of every pool's frame, in one Series (handler order)."""
        best = self.best()
        above = (self.best_option >= 0) & (self.best_prob > np.float32(threshold))
        return best['option'][above]

    def doublet_probability(self) -> pd.Series:
        """Per barcode the posterior mass of its pool's pair options, float64, added in ascending option order (0 for a run
        without doublets, NaN for a barcode in no pool)."""
        return pd.Series(self.doublet_mass, index=self._index(self.barcodes))
