"""Posteriors within per-barcode donor pools (Demultiplexer.predict_posteriors_in_pools).

A pool is a lane, hashtag group or sub-experiment that holds a known subset of the donors of one genotype table.  Each barcode
is scored against the donors of its own pool only, so its row has the pool's options - the singlets of the pool's donors in
genotype order, then their pairs - and the rows of different pools have different lengths.  The result is therefore COMPACT: one
flat float32 array per matrix and a row pointer, host-resident.  Per pool it unfolds into the DataFrames the reference returns for
that genotype sub-list.
"""
import numpy as np
import pandas as pd

from . import donor_readout


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


def pooled_layout(pools, pool_of_barcode, with_doublets):
    """The host layout of a pooled call (include/demux_hip_debug.h: dmx_estep_pools) from one list of table columns per pool and
    pool_of_barcode: (pool_start int64[n_pools + 1], the lists flat as int32, row_ptr int64[B + 1]).  A barcode's row has the options
    of its pool; an id that is no pool's - -1, in no pool, or any other, which the library refuses - has a row of length 0."""
    sizes = np.array([len(d) for d in pools], dtype=np.int64)
    pool_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    donors = np.ascontiguousarray(np.concatenate([np.asarray(d, dtype=np.int64).reshape(-1) for d in pools]) if len(pools) else [],
                                  dtype=np.int32)
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
    n_options = sizes * (sizes + 1) // 2 if with_doublets else sizes
    in_pool = (pool_of_barcode >= 0) & (pool_of_barcode < len(pools))
    row_len = np.zeros(len(pool_of_barcode), dtype=np.int64)
    row_len[in_pool] = n_options[pool_of_barcode[in_pool]]
    row_ptr = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    return pool_start, donors, row_ptr


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


class DevicePooledPosteriors:
    """Logits and posteriors of one pooled call (`on_device=True`), compact and kept on the GPU in the pooled slot of a private device
    context, with the reductions users apply to the per-pool frames done there: nothing of the size of the rows
    crosses the link unless to_dataframes() / to_host() ask for it.  Option indices and names are those of the barcode's own pool.
    close() (or the context manager) gives the context back.

    best_option / best_prob / doublet_mass: the B-sized read-outs of the pass itself, as PooledPosteriors holds them."""

    def __init__(self, ctx, barcodes, pool_names, pool_columns, pool_sizes, pool_of_barcode, row_ptr, best_option, best_prob, doublet_mass,
                 index_name='BARCODE', release=None):
        self._ctx = ctx
        self._release = release  # what close() does with the context (None: ctx.close())
        self.barcodes = list(barcodes)
        self._pool_names = list(pool_names)
        self._pool_columns = [list(c) for c in pool_columns]
        self._pool_sizes = [int(g) for g in pool_sizes]
        self.pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int32)
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.best_option = np.asarray(best_option, dtype=np.int32)
        self.best_prob = np.asarray(best_prob, dtype=np.float32)
        self.doublet_mass = np.asarray(doublet_mass, dtype=np.float64)
        self.index_name = index_name
        B = len(self.barcodes)
        assert len(self._pool_names) == len(self._pool_columns) == len(self._pool_sizes)
        assert self.pool_of_barcode.shape == (B,) and self.row_ptr.shape == (B + 1,)
        info = ctx.pooled_info()
        assert info['present'] and info['B'] == B and info['n_pools'] == len(self._pool_names), 'the context holds another result'
        self._opt_ptr = np.concatenate([[0], np.cumsum([len(c) for c in self._pool_columns])]).astype(np.int64)
        self._rows_of = [np.flatnonzero(self.pool_of_barcode == p) for p in range(len(self._pool_names))]

    # ---- layout -----------------------------------------------------------------------------------------------------------
    @property
    def pools(self):
        return list(self._pool_names)

    def _index(self, barcodes=None):
        index = pd.Index(self.barcodes if barcodes is None else barcodes)
        index.name = self.index_name
        return index

    def _pool_index(self, pool):
        if pool not in self._pool_names:
            raise KeyError(f'unknown pool {pool!r}')
        return self._pool_names.index(pool)

    def columns_of(self, pool):
        """The option names of a pool: its donors in genotype order, then 'A+B' for A before B."""
        return list(self._pool_columns[self._pool_index(pool)])

    def donors_of(self, pool):
        p = self._pool_index(pool)
        return self._pool_columns[p][:self._pool_sizes[p]]

    def barcodes_of(self, pool):
        """The pool's barcodes, in handler order."""
        return [self.barcodes[i] for i in self._rows_of[self._pool_index(pool)]]

    def _pool_labels(self):
        return np.asarray(self._pool_names + [None], dtype=object)[self.pool_of_barcode]

    def _option_labels(self, options):
        """object array of option names for pool-local indices (any shape with B first; -1: None)."""
        options = np.asarray(options)
        out = np.full(options.shape, None, dtype=object)
        for p, rows in enumerate(self._rows_of):
            names = np.asarray(self._pool_columns[p] + [None], dtype=object)
            out[rows] = names[options[rows]]
        return out

    # ---- the matrices ------------------------------------------------------------------------------------------------------
    def to_dataframes(self, pool):
        """(logits_df, probs_df) of one pool, as PooledPosteriors.to_dataframes: each gathered on the device, one download."""
        p = self._pool_index(pool)
        n, columns = len(self._rows_of[p]), self._pool_columns[p]
        barcodes = self.barcodes_of(pool)
        return tuple(pd.DataFrame(self._ctx.pooled_get_pool(what, p, n, len(columns)), index=self._index(barcodes), columns=columns)
                     for what in ('logits', 'probs'))

    def to_host(self) -> PooledPosteriors:
        """The whole result as the host-resident PooledPosteriors of the same call."""
        n = int(self.row_ptr[-1]) if len(self.barcodes) else 0
        logits, probs = (self._ctx.pooled_get(what, 0, len(self.barcodes), n) for what in ('logits', 'probs'))
        return PooledPosteriors(self.barcodes, self._pool_names, self._pool_columns, self.pool_of_barcode, self.row_ptr, logits, probs,
                                self.best_option, self.best_prob, self.doublet_mass, index_name=self.index_name)

    # ---- per barcode -------------------------------------------------------------------------------------------------------
    def best(self) -> pd.DataFrame:
        """Per barcode (all of them, handler order): its pool, the most probable option of the pool and its posterior; None /
        None / NaN for a barcode in no pool."""
        r = self._ctx.pooled_readout(masses=False)
        return pd.DataFrame({'pool': self._pool_labels(), 'option': self._option_labels(r['best_option']), 'probability': r['best_prob']},
                            index=self._index())

    def assignments(self, threshold=0.9) -> pd.Series:
        """probs[probs.max(axis=1).gt(threshold)].idxmax(axis=1) of every pool's frame, in one Series (handler order)."""
        r = self._ctx.pooled_readout(masses=False)
        with np.errstate(invalid='ignore'):
            above = (r['best_option'] >= 0) & (r['best_prob'] > np.float32(threshold))
        return pd.Series(self._option_labels(r['best_option']), index=self._index(), name='option')[above]

    def top_options(self, k=2) -> pd.DataFrame:
        """The k <= 4 best options per barcode, best first: columns pool, option_1, probability_1, option_2, ... (None / NaN where
        the pool has fewer options, or the barcode no pool)."""
        options, probs = self._ctx.pooled_top_options(k)
        names = self._option_labels(options)
        data = {'pool': self._pool_labels()}
        for j in range(options.shape[1]):
            data[f'option_{j + 1}'] = names[:, j]
            data[f'probability_{j + 1}'] = probs[:, j]
        return pd.DataFrame(data, index=self._index())

    def doublet_probability(self) -> pd.Series:
        """Per barcode the posterior mass of its pool's pair options, float64, added in ascending option order (0 for a run
        without doublets, NaN for a barcode in no pool)."""
        return pd.Series(self._ctx.pooled_readout()['doublet_mass'], index=self._index())

    def donor_marginals(self, pool) -> pd.DataFrame:
        """float32, the pool's barcodes x the pool's donors: the posterior mass of every option that contains the donor, added in
        float64 in ascending option order and rounded once."""
        p = self._pool_index(pool)
        r = self._ctx.pooled_readout(marginals=True)
        g, rows = self._pool_sizes[p], self._rows_of[p]
        take = (r['marg_ptr'][rows][:, None] + np.arange(g, dtype=np.int64)[None, :]).reshape(-1)
        return pd.DataFrame(r['donor_marginals'][take].reshape(len(rows), g), index=self._index(self.barcodes_of(pool)), columns=self.donors_of(pool))

    def droplet_calls(self, threshold=0.9) -> pd.DataFrame:
        """DevicePosteriors.droplet_calls per barcode with its own pool's donor names (donor_readout.compose_calls), plus a `pool`
        column; all barcodes, handler order.  A barcode in no pool is 'unassigned' with no donors and NaN probabilities."""
        r = self._ctx.pooled_readout()
        return self._compose_calls(r, threshold)

    def _compose_calls(self, r, threshold):
        B = len(self.barcodes)
        frame = pd.DataFrame({'status': np.full(B, 'unassigned', dtype=object), 'donor_1': np.full(B, None, dtype=object),
                              'donor_2': np.full(B, None, dtype=object), 'probability': np.full(B, np.nan), 'doublet_probability': np.full(B, np.nan)},
                             index=self._index())
        for p, rows in enumerate(self._rows_of):
            if len(rows) == 0:
                continue
            calls = donor_readout.compose_calls(self._pool_columns[p][:self._pool_sizes[p]], threshold, r['best_singlet'][rows],
                                                r['best_singlet_prob'][rows], r['best_pair'][rows], r['doublet_mass'][rows])
            for column in frame.columns:
                frame[column].values[rows] = calls[column].values
        frame.insert(0, 'pool', self._pool_labels())
        return frame

    # ---- per pool ----------------------------------------------------------------------------------------------------------
    def _all_option_sums(self):
        return self._ctx.pooled_option_sums(int(self._opt_ptr[-1]))[0]

    def option_sums(self, pool) -> pd.Series:
        """probs.sum(axis=0) of the pool's frame, float64 (zeros for a pool without barcodes)."""
        p = self._pool_index(pool)
        return pd.Series(self._all_option_sums()[self._opt_ptr[p]:self._opt_ptr[p + 1]], index=self._pool_columns[p])

    def donor_summary(self, threshold=0.9) -> pd.DataFrame:
        """Indexed by (pool, donor): n_singlets, n_doublets and expected_cells as DevicePosteriors.donor_summary forms them inside
        every pool - expected_cells from the pool's option sums, so nothing of the size of the rows is downloaded."""
        calls = self.droplet_calls(threshold)
        sums = self._all_option_sums()
        frames = []
        for p, rows in enumerate(self._rows_of):
            donors = self._pool_columns[p][:self._pool_sizes[p]]
            summary = donor_readout.compose_summary(donors, calls.iloc[rows], sums[self._opt_ptr[p]:self._opt_ptr[p + 1]])
            summary.index = pd.MultiIndex.from_product([[self._pool_names[p]], donors], names=['pool', 'donor'])
            frames.append(summary)
        return pd.concat(frames) if frames else pd.DataFrame(columns=['n_singlets', 'n_doublets', 'expected_cells'])

    def qualities(self, barcode2possible_options) -> dict:
        """DevicePosteriors.qualities with every name resolved inside the barcode's own pool.  Barcodes in no pool are left out of
        the means (they need no entry in the dict).  ValueError: a pooled barcode that is missing from the dict, a name that is not
        an option of the barcode's pool."""
        start = np.zeros(len(self.barcodes) + 1, dtype=np.int64)
        flat = []
        positions = [{name: k for k, name in enumerate(columns)} for columns in self._pool_columns]
        for b, barcode in enumerate(self.barcodes):
            p = self.pool_of_barcode[b]
            if p >= 0:
                if barcode not in barcode2possible_options:
                    raise ValueError(f'barcode {barcode!r} is not in barcode2possible_options')
                options = list(barcode2possible_options[barcode])
                unknown = [o for o in options if o not in positions[p]]
                if unknown:
                    raise ValueError(f'some of the options of {barcode!r} are not options of its pool {self._pool_names[p]!r}: {unknown}')
                flat.extend(positions[p][o] for o in options)
            start[b + 1] = len(flat)
        mass, hit = self._ctx.pooled_allowed_mass(start, np.asarray(flat, dtype=np.int32))
        pooled = self.pool_of_barcode >= 0
        return donor_readout.compose_qualities(mass[pooled], hit[pooled])

    # ---- life cycle --------------------------------------------------------------------------------------------------------
    def close(self):
        if self._ctx is not None:
            if self._release is not None:
                self._release(self._ctx)
            else:
                self._ctx.close()
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
